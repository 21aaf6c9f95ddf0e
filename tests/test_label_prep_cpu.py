""" CPU tests of the KITTI keypoint-label preparation (utils/label_prep.py, csrc/label_prep.hip's host side): the NumPy host
form against the scalar restatement of the MATLAB scripts (tests/label_prep_oracle.py) on every column, the text of the files, the C ABI's
argument checks (host code: they come before any launch), and the round trip that pins the conventions: labels -> prepared keypoints ->
the polling oracle (oracle/polling_np.py) -> utils.gpp_utils.recover_pose -> the labels' own location, dimensions and r_y.

The host form and the oracle share np.cos / np.sin and are otherwise the same IEEE double operations in the same order: equal, not close. """
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import label_prep_oracle as LO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.preprocessing import kitti
from keras_retinanet_3D.utils import gpp_utils, kitti_eval, synthetic
from keras_retinanet_3D.utils import label_prep as L
from oracle import polling_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_PLAIN = np.array([[700.0, 0.0, 600.0, 0.0], [0.0, 700.0, 180.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


def same(got, want):
    """ equal in every column (NaN nowhere) """
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert not np.isnan(want).any()
    bad = np.argwhere(got != want)
    assert bad.size == 0, 'first difference at {}: {!r} != {!r}'.format(bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------- host form == oracle
@pytest.mark.parametrize('seed,offset', [(1, True), (2, False), (3, True)])
def test_seeded_scenes_equal_the_oracle(seed, offset):
    labels, P = LO.seeded_scene(seed, 64, P_offset=offset)
    want = LO.mod_rows(labels, P)
    same(L.prepare(labels, P), want)
    demoted = want[:, 19] == -1
    assert 2 <= demoted.sum() <= 20 and set(want[~demoted, 19]) == {0.0, 1.0, 2.0, 3.0}
    # the batched form that the kernel is compared with: the same rows, -1 beyond the count
    mod, _ = L.prepare_batch(labels[None], [40], P[None])
    same(mod[0, :40], want[:40])
    assert (mod[0, 40:] == -1).all()


def test_hand_worked_object():
    """ r_y = 0, P = [700 0 600 0; 0 700 180 0; 0 0 1 0], h w l = 1.5 2 4 at (2, 1.5, 10): the bottom corners 1..4 lie at (X, Z) =
    (4, 11) (4, 9) (0, 9) (0, 11), u = 700 X / Z + 600, v = 700 Y / Z + 180 with Y = 1.5 (bottom) or 0 (top).  alpha = -0.2 rad is class 2:
    l m r t = corners 4 3 2 7 """
    g = LO.make_label(kind=0, trunc=0.25, occ=1, alpha=-0.2, box=(1.0, 2.0, 3.0, 4.0), hwl=(1.5, 2.0, 4.0), xyz=(2.0, 1.5, 10.0), ry=0.0)
    u1, u2, u34 = 9400.0 / 11.0, 8200.0 / 9.0, 600.0
    v_far, v_near, v_top = (1050.0 + 180.0 * 11.0) / 11.0, (1050.0 + 180.0 * 9.0) / 9.0, 180.0
    want = np.array([[0.0, 0.25, 1.0, -0.2, u34, v_top, u2, v_near,
                      u34, v_far, u34, v_near, u2, v_near, u34, v_top, 1.5, 2.0, 4.0, 2.0]])
    same(L.prepare(g, P_PLAIN), want)
    same(LO.mod_rows(g, P_PLAIN), want)
    # the same object seen under each class: the keypoints walk round the bottom face
    expected = {0.2: [u34, v_near, u2, v_near, u1, v_far, u2, v_top], 2.0: [u2, v_near, u1, v_far, u34, v_far, u1, v_top],
                -2.0: [u1, v_far, u34, v_far, u34, v_near, u34, v_top]}
    for alpha, kp in expected.items():
        g[3] = alpha
        got = L.prepare(g, P_PLAIN)
        same(got, LO.mod_rows(g, P_PLAIN))
        assert got[0, 8:16].tolist() == kp and got[0, 19] == {0.2: 0, 2.0: 1, -2.0: 3}[alpha]


def test_dont_care_rows_are_demoted_and_keep_their_box():
    labels = np.stack([LO.dont_care(), LO.make_label(alpha=1.0), LO.dont_care(box=(0.0, 0.0, 50.0, 60.5))])
    got = L.prepare(labels, synthetic.KITTI_LIKE_P2)
    same(got, LO.mod_rows(labels, synthetic.KITTI_LIKE_P2))
    for k, box in ((0, [503.0, 169.0, 590.0, 190.0]), (2, [0.0, 0.0, 50.0, 60.5])):
        assert got[k].tolist() == [2.0, -1.0, -1.0, -10.0] + box + [-10000.0] * 8 + [-1.0, -1.0, -1.0, -1.0]
    assert got[1, 19] == 0 and got[1, 0] == 0


def test_the_depth_rule_at_its_boundary():
    """ r_y = 0 and w = 2^-5: the nearest corners lie at Z = t_z - 2^-6, exact for t_z next to 0.1 -- at exactly 0.1 the object is kept
    (the rule is Z < 0.1), at the next double below it is demoted """
    hw = 2.0 ** -6
    below = np.nextafter(0.1, 0.0)
    at, under = LO.make_label(alpha=0.5, hwl=(1.5, 2 * hw, 0.5), xyz=(0.0, 1.6, 0.1 + hw)), LO.make_label(alpha=0.5, hwl=(1.5, 2 * hw, 0.5), xyz=(0.0, 1.6, below + hw))
    assert (-hw) + at[13] == 0.1 and (-hw) + under[13] == below and below < 0.1
    got = L.prepare(np.stack([at, under]), P_PLAIN)
    same(got, LO.mod_rows(np.stack([at, under]), P_PLAIN))
    assert got[0, 19] == 0 and got[0, 0] == 0 and np.isfinite(got[0]).all()
    assert got[1, 19] == -1 and got[1, 0] == 2 and (got[1, 8:16] == -10000).all()


def test_the_class_boundaries_of_alpha():
    """ -pi, 0 and the doubles on either side of +-pi/2; deg = (180 / pi) alpha decides, as rad2deg does """
    hp = math.pi / 2
    cases = [(-math.pi, 3), (0.0, 0), (np.nextafter(0.0, -1.0), 2), (np.nextafter(hp, 0.0), 0), (np.nextafter(hp, 4.0), 1),
             (np.nextafter(-hp, -4.0), 3), (np.nextafter(-hp, 0.0), 2), (np.nextafter(math.pi, 0.0), 1)]
    labels = np.stack([LO.make_label(alpha=a, xyz=(1.0, 1.6, 15.0), ry=0.3) for a, _ in cases])
    got = L.prepare(labels, synthetic.KITTI_LIKE_P2)
    same(got, LO.mod_rows(labels, synthetic.KITTI_LIKE_P2))
    assert got[:, 19].tolist() == [float(c) for _, c in cases]
    # +-pi/2 themselves: (180 / pi) (pi / 2) is 90 exactly in double
    assert (180.0 / math.pi) * hp == 90.0
    both = L.prepare(np.stack([LO.make_label(alpha=hp), LO.make_label(alpha=-hp)]), synthetic.KITTI_LIKE_P2)
    assert both[:, 19].tolist() == [1.0, 2.0]


def test_an_image_without_labels():
    got = L.prepare(np.zeros((0, 16)), synthetic.KITTI_LIKE_P2)
    assert got.shape == (0, 20) and got.dtype == np.float64
    assert LO.mod_rows(np.zeros((0, 16)), synthetic.KITTI_LIKE_P2).shape == (0, 20)
    assert L.format_lines([], got) == ''
    mod, det = L.prepare_batch(np.zeros((2, 0, 16)), [0, 0], np.tile(synthetic.KITTI_LIKE_P2, (2, 1, 1)), det_types=L.CAR)
    assert mod.shape == (2, 0, 20) and det[0].shape == (2, 0, 12) and det[4].dtype == np.int32


@pytest.mark.parametrize('alpha', [math.pi, 3.5, -3.5, float('nan')])
def test_alpha_outside_the_range_raises(alpha):
    g = LO.make_label(alpha=alpha)
    with pytest.raises(ValueError):
        LO.mod_rows(g, synthetic.KITTI_LIKE_P2)
    with pytest.raises(ValueError):
        L.prepare(g, synthetic.KITTI_LIKE_P2)
    # the kernel's rule (strict=False): the row is demoted; behind the camera the angle is never looked at (a DontCare line has alpha -10)
    assert L.prepare(g, synthetic.KITTI_LIKE_P2, strict=False)[0].tolist() == [2.0, -1.0, -1.0, -10.0] + [0.0] * 4 + [-10000.0] * 8 + [1.5, 1.6, 4.0, -1.0]
    g[13] = -3.0
    same(L.prepare(g, synthetic.KITTI_LIKE_P2), LO.mod_rows(g, synthetic.KITTI_LIKE_P2))


def test_detection_layout_of_the_host_form():
    labels, P = LO.seeded_scene(5, 12)
    labels[:3, 0], labels[3] = (0, 1, 3), LO.dont_care()                   # a Car, a Van, a Cyclist, a DontCare line, then as seeded
    mod, (boxes, dims, scores, det_labels, orient) = L.prepare_batch(labels[None], [10], P[None], det_types=L.CAR | L.VAN, own_box=True)
    is_det = (mod[0, :, 19] >= 0) & (labels[:, 0] <= 1) & (np.arange(12) < 10)
    assert is_det.sum() >= 4 and (~is_det).sum() >= 3
    assert boxes.dtype == dims.dtype == scores.dtype == np.float32 and det_labels.dtype == orient.dtype == np.int32
    assert np.array_equal(boxes[0, is_det, :4], labels[is_det, 4:8].astype(np.float32))
    assert np.array_equal(boxes[0, is_det, 4:], mod[0, is_det, 8:16].astype(np.float32))
    assert np.array_equal(dims[0, is_det], labels[is_det, 8:11].astype(np.float32))
    assert (scores[0, is_det] == 1).all() and (det_labels[0, is_det] == 0).all() and np.array_equal(orient[0, is_det], mod[0, is_det, 19].astype(np.int32))
    for a in (boxes, dims, scores, det_labels, orient):
        assert (a[0, ~is_det] == -1).all()
    _, (prepared, _, _, _, o2) = L.prepare_batch(labels[None], [10], P[None], det_types=L.CAR, own_box=False)
    cars = is_det & (labels[:, 0] == 0)
    assert np.array_equal(prepared[0, cars, :4], mod[0, cars, 4:8].astype(np.float32)) and (o2[0, ~cars] == -1).all() and cars.sum() < is_det.sum()


# ---------------------------------------------------------------------------------------------------- files
def test_format_lines_against_typed_lines():
    g = np.stack([LO.make_label(kind=0, trunc=0.25, occ=1, alpha=-0.2, box=(1.0, 2.0, 3.0, 4.0), hwl=(1.5, 2.0, 4.0), xyz=(2.0, 1.5, 10.0)),
                  LO.dont_care(),
                  LO.make_label(kind=3, trunc=0.0, occ=2, alpha=1.57, box=(10.5, 20.25, 30.0, 40.0), hwl=(1.75, 0.5, 1.0), xyz=(-3.0, 1.5, -2.0))])
    text = L.format_lines(['Car', 'DontCare', 'Pedestrian'], L.prepare(g, P_PLAIN))
    assert text == (
        'Car 0.250000 1 -0.200000 600.000000 180.000000 911.111111 296.666667 600.000000 275.454545 600.000000 296.666667 '
        '911.111111 296.666667 600.000000 180.000000 1.500000 2.000000 4.000000 2\n'
        'DontCare -1.000000 -1 -10.000000 503.000000 169.000000 590.000000 190.000000 -10000.000000 -10000.000000 -10000.000000 '
        '-10000.000000 -10000.000000 -10000.000000 -10000.000000 -10000.000000 -1.000000 -1.000000 -1.000000 -1\n'
        'DontCare -1.000000 -1 -10.000000 10.500000 20.250000 30.000000 40.000000 -10000.000000 -10000.000000 -10000.000000 '
        '-10000.000000 -10000.000000 -10000.000000 -10000.000000 -10000.000000 1.750000 0.500000 1.000000 -1\n')
    with pytest.raises(ValueError):
        L.format_lines(['Car'], np.zeros((2, 20)))


def test_written_files_read_back_through_the_generator(tmp_path):
    label_dir, calib_dir = LO.write_dataset(tmp_path, LO.three_scenes())
    out_dir = os.path.join(str(tmp_path), 'mod')
    assert L.write_mod_labels(label_dir, calib_dir, out_dir) == 3
    assert sorted(os.listdir(out_dir)) == ['000000.txt', '000001.txt', '000002.txt'] and os.path.getsize(os.path.join(out_dir, '000001.txt')) == 0
    for f in ('000000.txt', '000002.txt'):
        names, rows = L.read_labels(os.path.join(label_dir, f))
        assert np.array_equal(rows, kitti_eval.read_label_file(os.path.join(label_dir, f))) and len(names) == rows.shape[0]
        P = L.read_calibration(os.path.join(calib_dir, f))
        mod = L.prepare(rows, P)
        same(mod, LO.mod_rows(rows, P))
        rounded = np.array([float('%f' % v) for v in mod.ravel()]).reshape(mod.shape)
        objects, ignore = kitti.parse_label_file(os.path.join(out_dir, f))
        keep = np.array([(n in kitti.kitti_classes) and m[19] >= 0 for n, m in zip(names, mod)])
        gone = np.array([n in kitti.IGNORED_TYPES or m[19] < 0 for n, m in zip(names, mod)])
        assert keep.sum() >= 2 and gone.sum() >= 1
        assert np.array_equal(objects[:, :15], rounded[keep][:, 4:19]) and np.array_equal(objects[:, 16], mod[keep][:, 19]) and (objects[:, 15] == 0).all()
        assert np.array_equal(ignore, rounded[gone][:, 4:8])


def test_an_out_of_range_alpha_in_a_file_names_the_file(tmp_path):
    scenes = LO.three_scenes()
    scenes[2][1][0, 3], scenes[2][1][0, 13] = 3.15, 20.0
    label_dir, calib_dir = LO.write_dataset(tmp_path, scenes)
    with pytest.raises(ValueError, match='000002.txt'):
        L.write_mod_labels(label_dir, calib_dir, os.path.join(str(tmp_path), 'mod'))


def test_command_line_writes_the_files_of_write_mod_labels(tmp_path, capsys):
    from keras_retinanet_3D.bin import polling_ceiling, prepare_labels
    label_dir, calib_dir = LO.write_dataset(tmp_path, LO.three_scenes())
    a, b = os.path.join(str(tmp_path), 'a'), os.path.join(str(tmp_path), 'b')
    prepare_labels.main([label_dir, calib_dir, a])
    assert '3 label files' in capsys.readouterr().out
    L.write_mod_labels(label_dir, calib_dir, b)
    for f in ('000000.txt', '000001.txt', '000002.txt'):
        assert open(os.path.join(a, f)).read() == open(os.path.join(b, f)).read()
    assert len(open(os.path.join(a, '000000.txt')).read().splitlines()) == 7
    args = polling_ceiling.parse_args([label_dir, calib_dir, 'a.mat', 'b.mat', '--json', 'out.json'])
    assert args.databases == ['a.mat', 'b.mat'] and args.image_dir is None and args.min_overlap == [0.7, 0.7, 0.7]
    with pytest.raises(SystemExit):
        polling_ceiling.parse_args([label_dir, calib_dir])


# ---------------------------------------------------------------------------------------------------- ABI
def test_abi_exports_label_prep_and_checks_arguments_before_any_launch():
    lib = hip.lib()
    assert hasattr(lib, 'gpp_label_prep_f64')
    header = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    assert int(re.search(r'#define GPP_LABEL_MOD_COLS (\d+)', header).group(1)) == hip.GPP_LABEL_MOD_COLS == L.MOD_COLS == 20
    assert int(re.search(r'#define GPP_KITTI_LABEL_COLS (\d+)', header).group(1)) == hip.GPP_KITTI_LABEL_COLS == kitti_eval.LABEL_COLS == 16
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda ins, B, A, mod, outs: lib.gpp_label_prep_f64(*(ins + [B, A, 1, 1, mod] + outs + [None]))  # noqa: E731
    ok, five, none = [p] * 4, [p] * 5, [None] * 5
    assert call(ok, -1, 4, p, five) == -1 and call(ok, 1, -4, p, none) == -1          # GPP_ERR_BAD_ARG
    for k in range(4):
        ins = list(ok)
        ins[k] = None
        assert call(ins, 1, 1, p, five) == -1 and call(ins, 1, 1, p, none) == -1, k
    assert call(ok, 1, 1, None, five) == -1
    for k in range(5):                                                                # all five detection arrays, or none
        outs = list(five)
        outs[k] = None
        assert call(ok, 1, 1, p, outs) == -1, k
        assert call(ok, 0, 1, p, outs) == -1, k
    assert call(ok, 0, 8, p, five) == 0 and call(ok, 8, 0, p, none) == 0              # nothing to do: GPP_OK, nothing launched
    assert call([None] * 4, 0, 0, None, none) == 0


def test_device_entry_points_fail_loudly_without_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    labels, P = LO.seeded_scene(1, 4)
    with pytest.raises(hip.GppError):
        L.prepare_device([labels], [P])
    label_dir, calib_dir = LO.write_dataset(tmp_path, LO.three_scenes())
    with pytest.raises(hip.GppError):
        L.polling_ceiling(label_dir, calib_dir, synthetic.load_plane_database('10'))
    with pytest.raises(hip.GppError):
        L.write_mod_labels(label_dir, calib_dir, os.path.join(str(tmp_path), 'mod'), device=True)


# ---------------------------------------------------------------------------------------------------- the round trip
def test_round_trip_through_polling_and_pose_returns_the_labels():
    """ The convention pin: 200 seeded objects at z = 6 .. 70 m under a KITTI-like P with a zero 4th column; their prepared keypoints,
    polled (oracle/polling_np.py, float32 as the reference) against the shipped 100 planes plus the object's own plane (0, -1, 0, t_y),
    must pick that plane -- every object, no exclusion -- and recover_pose must return the label's location and h, l within 1e-3 m and
    r_y within 1e-3 rad.  1e-3 m is the project's corner bar inside 100 m (utils/ledger.py); the reference chain alone was measured at
    4.9e-5 m / 2.5e-5 rad / 9.0e-5 m over 2 000 such objects.  Seed 7 is the first one tried. """
    n = 200
    labels, P = LO.seeded_scene(7, n, P_offset=False, kinds=(0,), behind=0.0)
    mod, (boxes, dims, _, _, orient) = L.prepare_batch(labels[:, None], np.ones(n, np.int32), np.tile(P, (n, 1, 1)), det_types=L.CAR, own_box=False)
    assert (orient >= 0).all() and sorted(set(orient.ravel().tolist())) == [0, 1, 2, 3]
    database = synthetic.load_plane_database('100').astype(np.float32)
    planes = np.tile(np.concatenate([database, np.zeros((1, 4), np.float32)])[None], (n, 1, 1))
    planes[:, -1] = np.stack([np.zeros(n), -np.ones(n), np.zeros(n), labels[:, 12]], axis=1)
    P_inv = np.tile(np.linalg.pinv(P).astype(np.float32), (n, 1, 1))
    keypoints, keyplanes, residuals, index = polling_np.fit_road_planes(boxes, dims, orient, P_inv, planes, return_index=True)
    assert (index[:, 0] == database.shape[0]).all(), 'objects off their own plane: {}'.format(np.flatnonzero(index[:, 0] != database.shape[0]).tolist())
    det = gpp_utils.recover_pose({'keypoints': keypoints.reshape(n, 12), 'orientations': orient[:, 0], 'dimensions': dims[:, 0]})
    loc_err = np.abs(det['locations'].astype(np.float64) - labels[:, 11:14]).max(axis=1)
    h_err, l_err = np.abs(det['dimensions'][:, 0] - labels[:, 8]), np.abs(det['dimensions'][:, 2] - labels[:, 10])
    ry_err = np.abs((det['angles'][:, 1].astype(np.float64) - labels[:, 14] + np.pi) % (2 * np.pi) - np.pi)
    tilt = np.abs(det['angles'][:, [0, 2]]).max()
    print('round trip: location {:.2e} m, h {:.2e} m, l {:.2e} m, r_y {:.2e} rad, off-axis rotation {:.2e} rad'.format(
        loc_err.max(), h_err.max(), l_err.max(), ry_err.max(), tilt))
    assert loc_err.max() <= 1e-3 and h_err.max() <= 1e-3 and l_err.max() <= 1e-3 and ry_err.max() <= 1e-3
