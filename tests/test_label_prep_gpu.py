""" The KITTI keypoint-label kernel on the GPU (csrc/label_prep.hip) against the NumPy host form (utils/label_prep.py), which
tests/test_label_prep_cpu.py holds to the scalar restatement of the MATLAB scripts; and the ceiling of polling end to end:
label prep -> polling -> pose -> KITTI's Car benchmark, all on the device.

The kernel takes cos / sin from the host and is otherwise + - * /, minimum, maximum and compares in the host form's order, compiled without
contraction: every output is compared for equality, float64 and float32 alike. """
import filecmp
import os

import numpy as np
import pytest
import torch

import label_prep_oracle as LO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.bin import polling_ceiling, prepare_labels
from keras_retinanet_3D.utils import kitti_eval, synthetic
from keras_retinanet_3D.utils import label_prep as L

pytestmark = pytest.mark.gpu


def mixed_batch(B, A, counts, seed):
    """ labels (B, A, 16) of mixed types with objects behind the camera, DontCare lines, one alpha out of range and, beyond the counts,
    rows that are not zero; per image its own P (with and without the 4th column) """
    labels, P = np.empty((B, A, 16)), np.empty((B, 3, 4))
    for b in range(B):
        labels[b], P[b] = LO.seeded_scene(seed + b, A, P_offset=(b % 2 == 0), behind=0.15)
        labels[b, 1 % A] = LO.dont_care()
        labels[b, 2 % A, 3] = 3.3                                         # out of contract: the kernel demotes
    return labels, np.array(counts, np.int32), P


def run_kernel(labels, counts, P, det_types, own_box, detections=True):
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to('cuda')  # noqa: E731
    mod, det = hip.label_prep(up(labels), up(counts), up(P), up(L.trig_of(labels)), det_types, own_box, detections)
    torch.cuda.synchronize()
    return mod.cpu().numpy(), (None if det is None else tuple(t.cpu().numpy() for t in det))


SHAPES = {'B3_A8': (3, 8, [8, 3, 0]), 'B1_A128': (1, 128, [128]), 'B5_A60_two_blocks': (5, 60, [60, 61, -1, 7, 59])}


@pytest.fixture(scope='module')
def batches():
    return {name: mixed_batch(B, A, counts, 100 + 10 * k) for k, (name, (B, A, counts)) in enumerate(SHAPES.items())}


@pytest.mark.parametrize('det_types', [L.CAR, L.CAR | L.VAN | 8], ids=['cars', 'cars_vans_others'])
@pytest.mark.parametrize('own_box', [True, False], ids=['own_box', 'prepared_box'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_kernel_equals_the_host_form(batches, shape, own_box, det_types):
    labels, counts, P = batches[shape]
    want_mod, want_det = L.prepare_batch(labels, counts, P, det_types=det_types, own_box=own_box)
    mod, det = run_kernel(labels, counts, P, det_types, own_box)
    assert mod.dtype == np.float64 and not np.isnan(want_mod).any() and np.array_equal(mod, want_mod)
    for name, got, want in zip(('boxes', 'dims', 'scores', 'labels', 'orientations'), det, want_det):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    # the batch has what it is meant to have: valid rows of every class, demoted rows, padding, detections and non-detections
    live = np.arange(labels.shape[1])[None, :] < np.clip(counts, 0, labels.shape[1])[:, None]
    if shape != 'B3_A8':
        assert set(want_mod[live][:, 19].tolist()) == {-1.0, 0.0, 1.0, 2.0, 3.0}
    assert (want_mod[live][:, 19] == -1).any() and (want_mod[~live] == -1).all() and (~live).any() == (shape != 'B1_A128')
    assert 0 < (want_det[4] >= 0).sum() < live.sum()


def test_kernel_without_the_detection_arrays(batches):
    labels, counts, P = batches['B3_A8']
    mod, det = run_kernel(labels, counts, P, L.CAR, True, detections=False)
    assert det is None and np.array_equal(mod, L.prepare_batch(labels, counts, P)[0])


def test_prepare_device_returns_the_rows_of_prepare():
    scenes = LO.three_scenes()
    got = L.prepare_device([g for _, g, _ in scenes], [P for _, _, P in scenes])
    assert [m.shape for m in got] == [(7, 20), (0, 20), (5, 20)]
    for m, (_, g, P) in zip(got, scenes):
        assert np.array_equal(m, L.prepare(g, P))


# ---------------------------------------------------------------------------------------------------- the ceiling, end to end
T_Y = 1.65


def ceiling_scenes():
    """ three images of up to 8 Cars, Vans and DontCare lines on the plane y = 1.65, none behind the camera """
    scenes = []
    for seed, n in ((21, 8), (22, 5), (23, 7)):
        labels, P = LO.seeded_scene(seed, n, P_offset=False, kinds=(0, 0, 0, 1), behind=0.0)
        labels[:, 12] = T_Y
        labels[n - 1] = LO.dont_care(box=(20.0, 30.0, 90.0, 100.0))
        scenes.append(([LO.NAMES[int(k)] for k in labels[:, 0]], labels, P))
    return scenes


@pytest.fixture(scope='module')
def ceiling(tmp_path_factory):
    label_dir, calib_dir = LO.write_dataset(tmp_path_factory.mktemp('ceiling'), ceiling_scenes())
    planes = np.array([[0.0, -1.0, 0.0, T_Y], [0.0, -1.0, 0.0, T_Y + 0.4]], np.float32)          # the objects' own plane and one 0.4 m lower
    result = L.polling_ceiling(label_dir, calib_dir, planes, return_rows=True)
    files = sorted(os.listdir(label_dir))
    return {'label_dir': label_dir, 'calib_dir': calib_dir, 'planes': planes, 'result': result,
            'labels': [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in files]}


def test_ceiling_returns_the_labels_poses(ceiling):
    """ the bars of the CPU round trip (tests/test_label_prep_cpu.py): location, h and l within 1e-3 m, r_y within 1e-3 rad """
    n = 0
    for rows, g in zip(ceiling['result']['rows'], ceiling['labels']):
        assert rows.shape == (g.shape[0], 36) and rows.dtype == np.float32
        car = g[:, 0] == 0
        assert (rows[car, 14] >= 0).all() and (rows[~car] == -1).all()
        r, g = rows[car].astype(np.float64), g[car]
        loc = np.abs(np.stack([r[:, 19], r[:, 31], r[:, 21]], axis=1) - g[:, 11:14]).max()
        h, l = np.abs(r[:, 16] - g[:, 8]).max(), np.abs(r[:, 18] - g[:, 10]).max()
        ry = np.abs((r[:, 32] - g[:, 14] + np.pi) % (2 * np.pi) - np.pi).max()
        print('ceiling rows: location {:.2e} m, h {:.2e} m, l {:.2e} m, r_y {:.2e} rad'.format(loc, h, l, ry))
        assert loc <= 1e-3 and h <= 1e-3 and l <= 1e-3 and ry <= 1e-3
        assert np.array_equal(r[:, 26:30], g[:, 4:8].astype(np.float32))                         # the label's own box, unclipped at 376 x 1242
        n += int(car.sum())
    s = ceiling['result']['summary']
    assert n >= 9 and s['detections'] == n and s['nan_share'] == 0.0 and s['images'] == 3 and s['planes'] == 2 and s['chunks'] == 1
    assert s['location_error_max_m'] <= 3 ** 0.5 * 1e-3 and s['r_y_error_max_rad'] <= 1e-3 and s['location_error_median_m'] <= s['location_error_max_m']


def test_ceiling_scores_every_counted_label(ceiling):
    """ no false positive, no miss, and every AP at the maximum its difficulty allows.  KITTI samples the precision at the recall
    thresholds it finds among the true positives' scores: n counted labels give at most n of the 41 sample points (for n <= 40 exactly n:
    the walk of recall_thresholds never skips while k / 40 < (k + 1) / n), so a perfect detector on n labels scores
    AP|R40 = 100 (n - 1) / 40 and AP|R11 = 100 ceil(n / 4) / 11 -- precision 1 at the points 0 .. n - 1, nothing beyond. """
    result = ceiling['result']
    counted = np.zeros(3, np.int64)
    for g in ceiling['labels']:
        counted += (kitti_eval.label_status(g)[0] == 0).sum(axis=1)
    assert 40 >= counted[2] >= counted[1] >= counted[0] > 0
    for d, difficulty in enumerate(kitti_eval.DIFFICULTIES):
        n = int(counted[d])
        for metric in kitti_eval.METRICS:
            e = result[(metric, difficulty)]
            print('{} {}: {} counted labels, AP|R40 {} AP|R11 {}'.format(metric, difficulty, n, e['ap_r40'], e['ap_r11']))
            assert e['tp'].tolist() == [n] * n and e['fp'].tolist() == [0] * n and e['fn'].tolist() == [0] * n, (metric, difficulty)
            assert e['ap_r40'] == 100.0 * (n - 1) / 40.0 and e['ap_r11'] == 100.0 * len(range(0, n, 4)) / 11.0, (metric, difficulty)
        assert abs(result[('aos', difficulty)]['aos_r40'] - result[('image', difficulty)]['ap_r40']) <= 1e-3 * result[('image', difficulty)]['ap_r40']


def same_results(got, want):
    for key, entry in want.items():
        if key in ('summary', 'rows'):
            continue
        for name, value in entry.items():
            if name.startswith('aos'):
                assert abs(got[key][name] - value) <= 1e-9, (key, name)
            else:
                assert np.array_equal(got[key][name], value), (key, name)


def test_ceiling_integers_equal_the_host_evaluation_of_the_fetched_rows(ceiling):
    want = kitti_eval.evaluate_rows(ceiling['result']['rows'], ceiling['labels'])
    same_results(ceiling['result'], want)
    assert set(want) == set(ceiling['result']) - {'summary', 'rows'}


def test_two_chunks_give_the_result_of_one(ceiling):
    two = L.polling_ceiling(ceiling['label_dir'], ceiling['calib_dir'], ceiling['planes'], return_rows=True, chunk_images=2)
    assert two['summary']['chunks'] == 2
    same_results(two, ceiling['result'])
    for a, b in zip(two['rows'], ceiling['result']['rows']):
        assert np.array_equal(a, b)
    assert {k: v for k, v in two['summary'].items() if k != 'chunks'} == {k: v for k, v in ceiling['result']['summary'].items() if k != 'chunks'}
    # without the rows only the summary's columns come down: the same summary
    light = L.polling_ceiling(ceiling['label_dir'], ceiling['calib_dir'], ceiling['planes'])
    assert 'rows' not in light and light['summary'] == ceiling['result']['summary']
    same_results(light, ceiling['result'])


# ---------------------------------------------------------------------------------------------------- the command line
def test_prepare_labels_device_writes_the_bytes_of_the_host_run(tmp_path):
    label_dir, calib_dir = LO.write_dataset(tmp_path, LO.three_scenes())
    host, device = os.path.join(str(tmp_path), 'host'), os.path.join(str(tmp_path), 'device')
    prepare_labels.main([label_dir, calib_dir, host])
    prepare_labels.main([label_dir, calib_dir, device, '--device'])
    names = sorted(os.listdir(host))
    assert names == sorted(os.listdir(device)) == ['000000.txt', '000001.txt', '000002.txt']
    match, mismatch, errors = filecmp.cmpfiles(host, device, names, shallow=False)
    assert match == names and not mismatch and not errors
    assert os.path.getsize(os.path.join(host, '000000.txt')) > 0 and os.path.getsize(os.path.join(host, '000001.txt')) == 0


def test_polling_ceiling_command_line_prints_one_line_per_database(ceiling, tmp_path, capsys):
    import json
    out = os.path.join(str(tmp_path), 'ceiling.json')
    paths = [synthetic.plane_database_path('10'), synthetic.plane_database_path('100')]
    polling_ceiling.main([ceiling['label_dir'], ceiling['calib_dir']] + paths + ['--json', out])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith('road_planes_database_10.mat') and ' 10 planes' in lines[0] and '100 planes' in lines[1]
    got = json.load(open(out))
    assert sorted(got) == sorted(paths)
    want = L.polling_ceiling(ceiling['label_dir'], ceiling['calib_dir'], paths[1])
    assert got[paths[1]]['summary'] == want['summary'] and got[paths[1]]['3d_moderate']['ap_r40'] == want[('3d', 'moderate')]['ap_r40']
    assert got[paths[1]]['image_hard']['tp'] == want[('image', 'hard')]['tp'].tolist()
