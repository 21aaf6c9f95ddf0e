""" GPU tests of HOTA: csrc/hota_eval.hip against the NumPy form (utils/hota_eval.py), which
tests/test_hota_cpu.py holds against the loop-written oracle, scipy and a float64 restatement of the definition -- equality of every
array (with its dtype), every integer and every ratio. """
import math

import numpy as np
import pytest
import torch

import hota_oracle as HO
import mot_oracle as O
from keras_retinanet_3D.utils import hota_eval as H
from keras_retinanet_3D.utils import kitti_eval
from keras_retinanet_3D.utils import mot_eval as M
from keras_retinanet_3D.utils import pair_tables as PT
from keras_retinanet_3D.utils import track as T
from test_mot_eval_gpu import drive, same_result

pytestmark = pytest.mark.gpu

CASES = O.named_cases()
# the sizes at which the kernels can go wrong: one cell; more labels than rows and the reverse; the lane boundary (a lane's second column
# starts at 64); the full matrix
SIZES = [(1, 1), (9, 4), (4, 9), (63, 63), (64, 64), (65, 65), (64, 66), (128, 128), (128, 97)]
S = 1 << 20


def same_hota(got, want):
    same_result(got, want)                                                              # (everything of section 4.29, 'hota' in the summaries included)
    for key in ('match', 'counts'):
        a, b = got['hota_frames'][key], want['hota_frames'][key]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), key
    assert len(got['hota_pairs']) == len(want['hota_pairs'])
    for a, b in zip(got['hota_pairs'], want['hota_pairs']):
        for key in ('P', 'gc', 'tc', 'A', 'hist'):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key
    assert [e['hota'] for e in got['sequences']] == [e['hota'] for e in want['sequences']] and got['all']['hota'] == want['all']['hota']


def both(labels, tracks, **options):
    host = M.evaluate_sequences(labels, tracks, hota=True, **options)
    device = M.evaluate_sequences(labels, tracks, device=True, hota=True, **options)
    same_hota(device, host)
    return device


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_cases_equal_the_host_form(name):
    labels, tracks, _, options = CASES[name]
    h = both(labels, tracks, **options)['all']['hota']
    if name == 'perfect':
        assert h['integers']['tp'] == [10] * 19 and h['hota'] == h['deta'] == h['assa'] == h['loca'] == 1.0
    if name == 'swap':
        assert h['integers']['tp'] == [10] * 19 and h['integers']['ass'] == [2 * ((9 * S) // 7) + 2 * ((4 * S) // 8)] * 19
    if name == 'threshold':
        assert h['integers']['tp'] == [2] * 9 + [1] + [0] * 9
    if name == 'ignored':
        assert all(h[key] is None for key in H.RATIOS)


def test_split_and_the_tie_that_alignment_breaks():
    got = both(*HO.split_case())
    h = got['all']['hota']
    assert h['thresholds']['hota'] == [math.sqrt(0.5)] * 19 and h['thresholds']['assa'] == [0.5] * 19 and h['thresholds']['deta'] == [1.0] * 19
    assert got['all']['mota'] == 1.0 - 1.0 / 6.0
    got = both(*HO.tie_case())
    assert got['frames']['match'][3].tolist() == [0] and got['hota_frames']['match'][3].tolist() == [1] and got['all']['ids'] == 1
    assert got['all']['hota']['thresholds']['deta'] == [0.8] * 19 and got['all']['hota']['thresholds']['assa'] == [1.0] * 19


@pytest.mark.parametrize('G,T', SIZES, ids=['{}x{}'.format(*s) for s in SIZES])
def test_sizes_equal_the_host_form(G, T):
    labels, tracks = O.dense(G * 131 + T, G, T)
    got = both([labels], [tracks])
    assert got['hota_frames']['counts'][0, 38:].tolist() == [G, T] and got['all']['hota']['integers']['tp'][0] >= min(G, T) // 2


def test_a_sequence_of_dense_frames():
    """ shared label and tracker ids over frames of 65 x 66, 128 x 128, 64 x 64 and 66 x 65: table rows and columns beyond 64, cells that
    several frames add to, an alignment table that decides among equal overlaps """
    got = both(*HO.dense_sequence())
    pairs = got['hota_pairs'][0]
    assert pairs['P'].shape == (128, 128) and pairs['gc'].max() == 4 and pairs['tc'].max() == 4 and (pairs['hist'].sum(axis=2) > 1).any()
    assert got['hota_frames']['counts'][:, 38:].tolist() == [[65, 66], [128, 128], [64, 64], [66, 65]]
    assert not np.array_equal(got['hota_frames']['match'], got['frames']['match'])     # (the alignment moved a pair)


def test_one_sequence_of_40_frames_with_tied_costs():
    labels, tracks = O.scene(31, frames=40, cars=12, quantum=16.0)
    got = both([labels], [tracks])
    assert got['all']['hota']['integers']['tp'][0] > 50 and 0.0 < got['all']['hota']['assa'] < 1.0


def test_sequences_of_unequal_length_whole_and_in_chunks(monkeypatch):
    """ in chunks of four frames the second sweep starts after the first has ended: a pass 2 that began before pass 1 had seen every chunk
    of a sequence would read an unfinished table and differ """
    scenes = [O.scene(41, frames=17, cars=9, quantum=16.0), (([], []), ([], [])), O.scene(42, frames=5, cars=20), O.dense(3, 30, 40)]
    labels, tracks = [s[0] for s in scenes], [s[1] for s in scenes]
    got = both(labels, tracks)
    assert got['seq_start'].tolist() == [0, 17, 17, 22, 23] and all(got['sequences'][1]['hota'][key] is None for key in H.RATIOS)
    monkeypatch.setattr(kitti_eval, 'OVERLAP_WORKSPACE_BYTES', 4 * 40 * 32 * 8 * 4)        # four frames to a chunk: the same result
    assert kitti_eval.chunk_images(40, 32) == 4
    same_hota(M.evaluate_sequences(labels, tracks, device=True, hota=True), got)


@pytest.mark.parametrize('metric', M.METRICS)
def test_every_metric(metric):
    labels, tracks = O.scene(7, frames=4, cars=6)
    got = both([labels], [tracks], metric=metric, min_overlap=0.25)
    assert got['all']['hota']['integers']['tp'][0] > 0 and got['params']['metric'] == metric


def test_no_rows_and_no_labels():
    labels, tracks = O.scene(8, frames=3, cars=4)
    none = ([np.zeros((0, 36), np.float32)] * 3, [np.zeros(0, np.int32)] * 3)
    h = both([labels], [none])['all']['hota']
    assert h['integers']['tp'] == [0] * 19 and h['integers']['fn'][0] > 0 and h['integers']['fp'] == [0] * 19 and h['hota'] == 0.0
    h = both([([np.zeros((0, 16))] * 3, [np.zeros(0, int)] * 3)], [tracks])['all']['hota']
    assert h['integers']['fn'] == [0] * 19 and h['integers']['fp'][0] > 0 and h['deta'] == 0.0


def test_tracker_tensors_are_scored_where_they_lie():
    labels, frames, removed = drive(5)
    rows, ids, _, _ = T.track_rows_device(torch.as_tensor(frames).cuda(), ('dist', 2.0))
    assert rows.is_cuda and ids.is_cuda
    got = M.evaluate_sequences([labels], [(rows, ids)], device=True, hota=True)
    same_hota(got, M.evaluate_sequences([labels], [(rows.cpu().numpy(), ids.cpu().numpy())], hota=True))
    h = got['all']['hota']
    # the tracker keeps every identity: what is missing is what was removed, and every association is perfect
    assert h['integers']['tp'] == [6 * 30 - removed] * 19 and h['integers']['fn'] == [removed] * 19 and h['integers']['fp'] == [0] * 19
    assert h['thresholds']['asspr'] == [1.0] * 19 and h['loca'] == 1.0 and 0.0 < h['hota'] < 1.0


def test_capped_workspace_is_a_value_error(monkeypatch):
    labels, tracks = O.scene(8, frames=3, cars=4)
    monkeypatch.setattr(PT, 'PAIR_TABLE_BYTES', 64)
    with pytest.raises(ValueError, match='device=False'):
        M.evaluate_sequences([labels], [tracks], device=True, hota=True)
    assert 'hota' not in M.evaluate_sequences([labels], [tracks], device=True)['all']   # (the cap is HOTA's alone)
