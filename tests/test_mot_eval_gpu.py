""" GPU tests of the tracking score: csrc/mot_eval.hip against the NumPy form (utils/mot_eval.py), which
tests/test_mot_eval_cpu.py holds against the loop-written oracle and scipy -- equality of every code, every integer and every ratio. """
import numpy as np
import pytest
import torch

import mot_oracle as O
from keras_retinanet_3D.utils import kitti_eval
from keras_retinanet_3D.utils import mot_eval as M
from keras_retinanet_3D.utils import track as T

pytestmark = pytest.mark.gpu

CASES = O.named_cases()
# the sizes at which the kernel can go wrong: one cell; more labels than rows and the reverse; the lane boundary (a lane's second column
# starts at 64); the full matrix; nothing admissible
SIZES = [(1, 1), (9, 4), (4, 9), (63, 63), (64, 64), (65, 65), (64, 66), (128, 128), (128, 97)]


def same_result(got, want):
    assert got['sequences'] == want['sequences'] and got['all'] == want['all'] and got['names'] == want['names']
    assert np.array_equal(got['seq_start'], want['seq_start'])
    for a, b in zip(got['trajectories'], want['trajectories']):
        assert np.array_equal(a['track_ids'], b['track_ids']) and np.array_equal(a['table'], b['table'])
    for key in ('match', 'label_outcome', 'row_outcome', 'counts'):
        assert got['frames'][key].dtype == want['frames'][key].dtype and np.array_equal(got['frames'][key], want['frames'][key]), key


def both(labels, tracks, **options):
    host = M.evaluate_sequences(labels, tracks, **options)
    device = M.evaluate_sequences(labels, tracks, device=True, **options)
    same_result(device, host)
    return device


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_cases_equal_the_host_form(name):
    labels, tracks, expect, options = CASES[name]
    got = both(labels, tracks, **options)
    for key, value in expect.items():
        assert got['sequences'][0][key] == value and got['all'][key] == value, key
    if name == 'optimal_beats_greedy':
        assert got['all']['tp'] == 2 and got['frames']['match'][0].tolist() == [0, 1]       # greedy finds one pair (test_mot_eval_cpu.py)
    if name == 'ties':
        assert got['frames']['match'][0].tolist() == [0, 1]


@pytest.mark.parametrize('G,T', SIZES, ids=['{}x{}'.format(*s) for s in SIZES])
def test_sizes_equal_the_host_form(G, T):
    labels, tracks = O.dense(G * 131 + T, G, T)
    got = both([labels], [tracks])
    assert got['frames']['counts'][0, 6:].tolist() == [G, T] and got['all']['tp'] >= min(G, T) // 2


def test_nothing_admissible():
    labels, tracks = O.dense(5, 6, 5, far=True)
    got = both([labels], [tracks])
    assert (got['all']['tp'], got['all']['fn'], got['all']['fp']) == (0, 6, 5) and got['frames']['counts'][0, 5] == 6 * M.BIG


@pytest.mark.parametrize('quantum', [16.0, 4.0])
def test_one_sequence_of_40_frames(quantum):
    """ quantum 16: many overlaps of a frame are equal -- the reduced costs tie and the first column must win """
    labels, tracks = O.scene(31, frames=40, cars=12, quantum=quantum)
    got = both([labels], [tracks])
    assert got['all']['tp'] > 50 and got['all']['ids'] > 0 and got['all']['frag'] > 0 and got['all']['fp'] > 0


def test_three_sequences_of_unequal_length(monkeypatch):
    scenes = [O.scene(41, frames=17, cars=9, quantum=16.0), (([], []), ([], [])), O.scene(42, frames=5, cars=20), O.dense(3, 30, 40)]
    labels, tracks = [s[0] for s in scenes], [s[1] for s in scenes]
    got = both(labels, tracks)
    assert got['seq_start'].tolist() == [0, 17, 17, 22, 23] and got['sequences'][1]['frames'] == 0 and got['sequences'][1]['mota'] is None
    monkeypatch.setattr(kitti_eval, 'OVERLAP_WORKSPACE_BYTES', 4 * 40 * 32 * 8 * 4)        # four frames to a chunk: the same result
    assert kitti_eval.chunk_images(40, 32) == 4
    same_result(M.evaluate_sequences(labels, tracks, device=True), got)


@pytest.mark.parametrize('metric', M.METRICS)
def test_every_metric(metric):
    """ r_y = 0 and boxes on a grid: the BEV and 3-D overlaps are the same float64 operations in both forms (csrc/rot_iou.h) """
    labels, tracks = O.scene(7, frames=4, cars=6)
    got = both([labels], [tracks], metric=metric, min_overlap=0.25, max_occlusion=1.0, min_height=40.0)
    assert got['all']['tp'] > 0 and got['params']['metric'] == metric


def test_no_rows_and_no_labels():
    labels, tracks = O.scene(8, frames=3, cars=4)
    none = ([np.zeros((0, 36), np.float32)] * 3, [np.zeros(0, np.int32)] * 3)
    got = both([labels], [none])
    assert got['all']['tp'] == 0 and got['all']['fn'] == got['all']['n_gt'] > 0
    got = both([([np.zeros((0, 16))] * 3, [np.zeros(0, int)] * 3)], [tracks])
    assert got['all']['n_gt'] == 0 and got['all']['fp'] > 0


def drive(seed, frames=30, cars=6, max_age=2):
    """ a scene of the kind tests/test_track_gpu.py tracks: cars in lanes 6 m apart, constant velocity along z, 5 cm of noise, every car
    missing in at most max_age consecutive frames; values of two decimals, so that the tracking text says what the rows say
    -> (labels, rows (N, D, 36) float32 with -1 padding, the number of rows removed) """
    rng = np.random.default_rng(seed)
    z0, vz = rng.uniform(20.0, 40.0, cars), rng.uniform(-0.5, 0.5, cars)
    run, removed = [0] * cars, 0
    labs, tids, rows = [], [], np.full((frames, cars + 2, 36), -1.0, np.float32)
    for f in range(frames):
        g, order, k_row = [], rng.permutation(cars + 2), 0
        for k in range(cars):
            lab = O.label(0, (100.0 + 150 * k, 100.0, 200.0 + 150 * k, 180.0))
            lab[9:14] = [1.75, 4.25, 6.0 * (k - cars / 2.0), 1.65, np.round(z0[k] + vz[k] * f, 2)]
            g.append(lab)
            if run[k] < max_age and rng.uniform() < 0.3:
                run[k] += 1
                removed += 1
                continue
            run[k] = 0
            seen = lab.copy()
            seen[11], seen[13] = np.round(seen[11] + rng.normal(0.0, 0.05), 2), np.round(seen[13] + rng.normal(0.0, 0.05), 2)
            rows[f, order[k_row]] = O.row_of(seen, score=0.75)
            k_row += 1
        labs.append(np.stack(g))
        tids.append(np.arange(cars) + 20)
    return (labs, tids), rows, removed


def test_tracker_tensors_are_scored_where_they_lie(tmp_path):
    labels, frames, removed = drive(5)
    rows, ids, hits, _ = T.track_rows_device(torch.as_tensor(frames).cuda(), ('dist', 2.0))
    assert rows.is_cuda and ids.is_cuda
    packed = M.pack_sequences([labels], [(rows, ids)])
    assert packed.rows.data_ptr() == rows.data_ptr() and packed.ids.data_ptr() == ids.data_ptr()        # no copy, no host
    got = M.evaluate_sequences([labels], [(rows, ids)], device=True)
    same_result(got, M.evaluate_sequences([labels], [(rows.cpu().numpy(), ids.cpu().numpy())]))
    # the end-to-end check: the tracker keeps every identity, and what is missing is exactly what was removed
    assert removed > 10 and got['all']['ids'] == 0 and got['all']['fn'] == removed and got['all']['fp'] == 0
    assert got['all']['tp'] == 6 * 30 - removed and got['all']['motp'] == 1.0 and got['all']['frag'] > 0
    bev = M.evaluate_sequences([labels], [(rows, ids)], device=True, metric='bev')
    assert (bev['all']['ids'], bev['all']['fn'], bev['all']['fp']) == (0, removed, 0) and 0.8 < bev['all']['motp'] < 1.0
    # the same tracks through the text: the same score
    with open(str(tmp_path / 'tracks.txt'), 'w') as f:
        for k in range(30):
            f.write(T.tracking_lines(k, rows[k].cpu().numpy(), ids[k].cpu().numpy(), hits[k].cpu().numpy()))
    kinds = {0: 'Car'}
    with open(str(tmp_path / 'labels.txt'), 'w') as f:
        for k, (g, t) in enumerate(zip(*labels)):
            for line, tid in zip(g, t):
                f.write('{} {} {} {:g} {:g} '.format(k, int(tid), kinds[int(line[0])], line[1], line[2]) + ' '.join(repr(float(v)) for v in line[3:15]) + '\n')
    for device in (False, True):
        text = M.evaluate_tracking(str(tmp_path / 'labels.txt'), str(tmp_path / 'tracks.txt'), device=device)
        assert text['all'] == got['all'] and text['sequences'] == got['sequences']
        assert all(np.array_equal(a['table'], b['table']) for a, b in zip(text['trajectories'], got['trajectories']))


def test_a_short_tensor_is_padded_to_the_labels():
    labels, frames, _ = drive(6, frames=6)
    rows, ids, _, _ = T.track_rows_device(torch.as_tensor(frames[:4]).cuda(), ('dist', 2.0))
    got = M.evaluate_sequences([labels], [(rows, ids)], device=True)
    same_result(got, M.evaluate_sequences([labels], [(rows.cpu().numpy(), ids.cpu().numpy())]))
    assert got['all']['frames'] == 6 and got['all']['fn'] >= 12
    with pytest.raises(ValueError, match='device=True'):
        M.evaluate_sequences([labels], [(rows, ids)])
