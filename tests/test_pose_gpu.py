"""
GPU tests of the device pose stage: gpp_pose_f32 (csrc/pose.hip) against the float64 oracle of tests/pose_oracle.py, the plan op
RetinaNet3D(pose=True) end to end, and bin/run_network.py --device-pose.

Yardstick of the kernel test: the deviation of the EXISTING host path (select_detections + recover_pose + the arithmetic of
kitti_lines, float32 intermediates) from the same oracle on the same rows, per field group.  The device computes in float64 and
rounds once, so per field group its largest deviation has to be at most max(the host path's largest deviation, 4 float32 ulp of the
oracle value); angles compare modulo 2 pi.  KITTI text: `%.2f` of a device field may differ from `%.2f` of the oracle value by one unit
of the last digit only, and no more fields may differ than differ for the host path.

Measured on an MI355X (the three resnet50 fixtures + both harness goldens, 8 045 rows; device rows / host path; the table is in
profiles/pose/README.md): locations 3.2e-3 / 3.2e-3 m and dimensions 8.9e-4 / 1.3e-3 m (half a float32 ulp of detections tens of
kilometres away), rotation vector 1.2e-7 / 1.6e-7, alpha 1.2e-7 / 2.2e-7, KITTI height 2.4e-4 / 8.8e-4, KITTI y 6.8e-6 / 1.4e-5;
`%.2f` fields differing from the oracle's text: 37 / 40 of 104 585, of which 2 / 5 in the eight pose fields.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import pose_oracle as O
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import gpp_utils, synthetic

pytestmark = pytest.mark.gpu

MEAN = np.array([103.939, 116.779, 123.68], np.float32)
POSE_FIELDS = (0, 5, 6, 7, 8, 9, 10, 11)            # of the 13 numbers of a KITTI line: alpha, h, w, l, x, y, z, r_y


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def text_fields(row):
    return ['%.2f' % v for v in O.kitti_fields(row)]


def one_unit_apart(a, b):
    """ two `%.2f` texts that differ by one unit of the last digit """
    return abs(int(round(float(a) * 100)) - int(round(float(b) * 100))) == 1


def test_kernel_against_the_float64_oracle_on_the_fixtures():
    differ = {'device': 0, 'host': 0, 'device_pose': 0, 'host_pose': 0}
    fields = rows_seen = 0
    worst = {}
    for fx in O.FIXTURES:
        outs, scales, shapes = O.fixture_outputs(fx)
        want, want_counts = O.pose_rows(outs, scales, shapes)
        host = O.host_rows(outs, scales, shapes)
        rows, counts = gpp_utils.recover_pose_device(outs, scales, shapes)
        assert rows.dtype == np.float32 and rows.shape == want.shape and counts.dtype == np.int32
        assert np.array_equal(counts, want_counts)
        valid = want[..., O.SCORE] > 0
        for b in range(want.shape[0]):                                   # the counted rows are a prefix
            assert valid[b, :counts[b]].all() and not valid[b, counts[b]:].any()
        assert (rows[~valid] == -1).all()
        assert np.isfinite(want[valid]).all() and np.isfinite(rows[valid]).all()         # none of these rows is degenerate
        assert (rows[valid][:, 33:] == 0).all()
        rows_seen += int(valid.sum())
        for name, cols, angular in O.GROUPS:
            d_dev = O.deviation(rows, want, cols, angular)[valid]
            d_host = O.deviation(host, want, cols, angular)[valid]
            bar = np.maximum(d_host.max(), 4 * O.ulp32(want[..., cols][valid]))
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], float(d_dev.max())), max(w[1], float(d_host.max()))
            print('{:36s} {:10s} device {:.3e}  host path {:.3e}'.format(fx, name, d_dev.max(), d_host.max()))
            assert (d_dev <= bar).all(), (fx, name, float(d_dev.max()), float(d_host.max()))
        for b in range(want.shape[0]):
            for r_w, r_h, r_d in zip(want[b, :counts[b]], host[b, :counts[b]], rows[b, :counts[b]]):
                for k, (a, h, d) in enumerate(zip(text_fields(r_w), text_fields(r_h), text_fields(r_d))):
                    fields += 1
                    if a != d:
                        assert one_unit_apart(a, d), (fx, b, k, a, d)
                        differ['device'] += 1
                        differ['device_pose'] += k in POSE_FIELDS
                    if a != h:
                        differ['host'] += 1
                        differ['host_pose'] += k in POSE_FIELDS
    print('rows {}, text fields {}: differing from the oracle text: {}'.format(rows_seen, fields, differ))
    for name, (d, h) in worst.items():
        print('worst {:10s} device {:.3e}  host path {:.3e}'.format(name, d, h))
    assert rows_seen == 8045
    # all 13 fields of a line, and the eight that come out of the pose arithmetic (the box fields and the score are one float32
    # division or none in both paths)
    assert differ['device'] <= differ['host'] and differ['device_pose'] <= differ['host_pose'], differ


def crafted_batch():
    """ B = 16 images x 12 detections: random but regular detections of all four orientation classes, then rows rewritten by hand """
    rng = np.random.default_rng(11)
    B, D = 16, 12
    X_m = rng.uniform(-20, 20, size=(B, D, 3)).astype(np.float32)
    X_m[..., 2] = rng.uniform(5, 80, size=(B, D))
    kp = np.empty((B, D, 4, 3), np.float32)
    kp[:, :, 1] = X_m
    kp[:, :, 0] = X_m + rng.normal(size=(B, D, 3)) * 2
    kp[:, :, 2] = X_m + rng.normal(size=(B, D, 3)) * 2
    kp[:, :, 3] = X_m + rng.normal(size=(B, D, 3)) * np.array([0.2, 1.0, 0.2]) - np.array([0, 1.5, 0])
    boxes = rng.uniform(0, 1200, size=(B, D, 12)).astype(np.float32)
    dims = rng.uniform(1, 5, size=(B, D, 3)).astype(np.float32)
    scores = np.sort(rng.uniform(0.06, 1, size=(B, D)).astype(np.float32), axis=1)[:, ::-1].copy()
    labels = np.zeros((B, D), np.int32)
    orient = rng.integers(0, 4, size=(B, D)).astype(np.int32)
    orient[0, :4] = [0, 1, 2, 3]
    residuals = rng.uniform(0, 2, size=(B, D)).astype(np.float32)
    keyplanes = np.zeros((B, D, 1, 4), np.float32)
    thr = np.float32(0.05)
    # image 1: the tail is padding, as decode writes it
    orient[1, 8:], scores[1, 8:], labels[1, 8:] = -1, -1, -1
    # image 2: scores at the threshold, one float32 below it and one above it
    scores[2, 9], scores[2, 10], scores[2, 11] = np.nextafter(thr, np.float32(1)), thr, np.nextafter(thr, np.float32(0))
    # image 3: zero-length edges -- X_t = X_m (row 4), X_l = X_m with orientation 0 (row 6), every keypoint the same (row 8)
    kp[3, 4, 3] = kp[3, 4, 1]
    orient[3, 6] = 0
    kp[3, 6, 0] = kp[3, 6, 1]
    kp[3, 8, :] = 1.0
    # image 4: [x y z] = 2 k k^T - I with k = (2, 1, 2) / 3, a rotation by exactly pi (row 2: orientation 0, l = 4.5, h = 2.25, every
    # coordinate exact in float32), and the same with one keypoint coordinate moved by one float32 ulp: within 1e-7 of pi (row 3)
    for d, y_t in ((2, np.float32(3.75)), (3, np.nextafter(np.float32(3.75), np.float32(4)))):
        orient[4, d] = 0
        kp[4, d] = [[1.5, 0, 16], [1, 2, 20], [7, 7, 7], [0, y_t, 19]]
    # image 5: the identity (no rotation at all: the s < 1e-5, c > 0 branch), orientation 1: x = (X_m - X_r) / l, y = (X_m - X_t) / h
    orient[5, 0] = 1
    kp[5, 0] = [[9, 9, 9], [2, 1, 30], [-2, 1, 30], [2, -0.5, 30]]
    # image 6: boxes that need each clipping side, and all of them
    boxes[6, 0, :4] = [-5, 10, 100, 200]
    boxes[6, 1, :4] = [5, -10, 100, 200]
    boxes[6, 2, :4] = [5, 10, 3000, 200]
    boxes[6, 3, :4] = [5, 10, 100, 1000]
    boxes[6, 4, :4] = [-3, -4, 3000, 1000]
    outs = [boxes, dims, scores, labels, orient, kp, keyplanes, residuals]
    scales = list(rng.uniform(0.5, 2.0, size=B))
    shapes = [(375, 1242, 3)] * B
    return outs, scales, shapes


def test_kernel_on_crafted_rows():
    """ the oracle decides every value; the host path decides where NaN may stand.  Bar where the issue sets none: the device value is
    a float64 result rounded once, so it is within half a float32 ulp of its own float64 value, which differs from the oracle's by
    float64 rounding of a few hundred operations on numbers no larger than the row's largest coordinate -- 4 float32 ulp of the oracle
    value + 1e-12 * (1 + the largest magnitude of the row) covers both (the second term matters where the oracle value is 0). """
    outs, scales, shapes = crafted_batch()
    want, want_counts = O.pose_rows(outs, scales, shapes)
    with np.errstate(all='ignore'):
        host = O.host_rows(outs, scales, shapes)
    rows, counts = gpp_utils.recover_pose_device(outs, scales, shapes)
    assert np.array_equal(counts, want_counts) and counts[1] == 8 and counts[2] == 10 and counts[0] == 12
    valid = want[..., O.SCORE] > 0
    assert (rows[~valid] == -1).all() and (rows[1, 8:] == -1).all() and (rows[2, 10:] == -1).all() and (rows[2, 9] != -1).any()
    # NaN exactly where the oracle has it, which is where the host path has it: the pose columns of the three degenerate rows
    assert np.array_equal(np.isnan(rows), np.isnan(want))
    nan_rows = sorted(zip(*np.where(np.isnan(want).any(axis=2))))
    assert nan_rows == [(3, 4), (3, 6), (3, 8)]
    for b, d in nan_rows:
        assert sorted(np.where(np.isnan(rows[b, d]))[0]) == O.POSE_COLS
        assert not np.isfinite(host[b, d, 19:26]).any()
    scale_of_row = np.nanmax(np.abs(want), axis=2, keepdims=True)
    bar = 4 * O.ulp32(np.nan_to_num(want)) + 1e-12 * (1 + scale_of_row)
    for name, cols, angular in O.GROUPS:
        d = O.deviation(rows, want, cols, angular)
        ok = (d <= bar[..., cols]) | np.isnan(want[..., cols])
        assert ok[valid].all(), (name, np.argwhere(~ok & valid[..., None])[:4], float(np.nanmax(d[valid])))
    # the rotation by pi and its neighbour: |rotation vector| = pi (to 1e-7), along +-(2, 1, 2) / 3
    for d in (2, 3):
        v = rows[4, d, 22:25].astype(np.float64)
        assert abs(np.linalg.norm(v) - np.pi) < 2e-7 and np.allclose(np.abs(v) / np.linalg.norm(v), [2 / 3, 1 / 3, 2 / 3], atol=1e-6)
    assert (rows[5, 0, 22:25] == 0).all() and np.allclose(rows[5, 0, 16:19], [1.5, outs[1][5, 0, 1], 4.0])
    # clipping, each side
    s6 = scales[6]
    assert rows[6, 0, 26] == 0 and rows[6, 1, 27] == 0 and rows[6, 2, 28] == 1242 and rows[6, 3, 29] == 375
    assert rows[6, 4, 26:30].tolist() == [0, 0, 1242, 375] and np.allclose(rows[6, 4, 0:4], np.array([-3, -4, 3000, 1000]) / s6)
    assert rows[6, 0, 27] == rows[6, 0, 1] and rows[6, 0, 28] == rows[6, 0, 2]
    assert set(np.unique(rows[0, :4, 14])) == {0, 1, 2, 3}


def test_empty_batches_and_bad_arguments():
    outs, scales, shapes = crafted_batch()
    empty_b = [o[:0] for o in outs]
    rows, counts = gpp_utils.recover_pose_device(empty_b, [], [(375, 1242, 3)])
    assert rows.shape == (0, 12, 36) and counts.shape == (0,)
    empty_d = [o[:, :0] for o in outs]
    rows, counts = gpp_utils.recover_pose_device(empty_d, scales, shapes)
    assert rows.shape == (16, 0, 36) and counts.tolist() == [0] * 16
    # tensors in -> tensors out, on the device
    dev = torch.device('cuda', torch.cuda.current_device())
    t_rows, t_counts = gpp_utils.recover_pose_device([torch.as_tensor(o).to(dev) for o in outs], scales, shapes)
    n_rows, n_counts = gpp_utils.recover_pose_device(outs, scales, shapes)
    assert t_rows.is_cuda and same_bytes(t_rows.cpu().numpy(), n_rows) and same_bytes(t_counts.cpu().numpy(), n_counts)
    lib = hip.lib()
    buf = torch.zeros((64,), dtype=torch.float32, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    ok = [p] * 8
    for args in ([-1, 1], [1, -1]):
        assert lib.gpp_pose_f32(*(ok + args + [0.05, p, p, None])) == -1           # GPP_ERR_BAD_ARG
    for k in range(8):
        a = list(ok)
        a[k] = None
        assert lib.gpp_pose_f32(*(a + [1, 1, 0.05, p, p, None])) == -1
    assert lib.gpp_pose_f32(*(ok + [1, 1, 0.05, None, p, None])) == -1 and lib.gpp_pose_f32(*(ok + [1, 1, 0.05, p, None, None])) == -1
    torch.cuda.synchronize()
    assert (buf == 0).all()                                                     # nothing was launched


@pytest.fixture(scope='module')
def weights50():
    return W.synthetic_weights('resnet50', 1234)


def frames(batch, h, w, seed):
    """ binary noise: keeps the synthetic weights' scores above the 0.05 threshold """
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, size=(batch, h, w, 3)) * 255).astype(np.float32) - MEAN


@pytest.mark.parametrize('dtype', ['f16x3', 'f32'])
@pytest.mark.parametrize('h,w,n_planes', [(96, 160, '100'), (402, 1333, '1k')])
def test_pose_model_end_to_end(weights50, dtype, h, w, n_planes, monkeypatch):
    monkeypatch.setenv('GPP_AUTOTUNE', '0')                  # (a tile never changes a byte: tests/test_network_gpu.py)
    B = 2
    plain = models.load_model(weights50, backbone_name='resnet50', dtype=dtype)
    posed = models.load_model(weights50, backbone_name='resnet50', dtype=dtype, pose=True)
    planes = synthetic.load_plane_database(n_planes).astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    inputs = [frames(B, h, w, seed=h), np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
    scale, shape = 402.0 / 375.0, (375, 1242, 3)
    want = plain.predict_on_batch(inputs)
    got = posed.predict_on_batch(inputs)
    assert len(got) == len(want) == 8
    for a, b in zip(got, want):
        assert same_bytes(a, b)
    rows, counts = posed.predict_poses_on_batch(inputs, scale, shape)
    assert rows.shape == (B, 100, 36) and rows.dtype == np.float32 and counts.shape == (B,) and counts.dtype == np.int32
    ref_rows, ref_counts = gpp_utils.recover_pose_device(got, [scale] * B, [shape] * B)
    assert same_bytes(rows, ref_rows) and same_bytes(counts, ref_counts)
    assert np.array_equal(counts, (got[2] > 0.05).sum(axis=1))
    if h == 402:
        assert counts.sum() > 0
    assert posed.range_fallbacks == 0 and plain.range_fallbacks == 0
    with pytest.raises(hip.GppError):
        plain.predict_poses_on_batch(inputs, scale, shape)
    if h != 402:
        return
    # per-image scales and shapes, then the same under a captured graph: frame_info is a buffer the graph reads
    scales2, shapes2 = [1.0, 1.5], [(375, 1242, 3), (370, 1224, 3)]
    rows2, counts2 = posed.predict_poses_on_batch(inputs, scales2, shapes2)
    ref2 = gpp_utils.recover_pose_device(got, scales2, shapes2)
    assert same_bytes(rows2, ref2[0]) and same_bytes(counts2, ref2[1])
    plan = posed.plan_for(B, h, w, planes.shape[0], True)
    posed.capture(plan)
    try:
        r3, c3 = posed.predict_poses_on_batch(inputs, scale, shape)
        assert same_bytes(r3, rows) and same_bytes(c3, counts)
        r4, c4 = posed.predict_poses_on_batch(inputs, scales2, shapes2)
        assert same_bytes(r4, rows2) and same_bytes(c4, counts2)
        assert not same_bytes(r4, r3)
    finally:
        plan.graph = None


def test_range_event_answers_with_the_twins_rows(weights50, monkeypatch):
    """ dtype='f16x3': a call whose activations leave the half range is answered by the float32 twin, rows included.  The weights of
    tests/test_range_reaction_gpu.py: bn2a_branch2a scaled by 2^17 and res2a_branch2b by 2^-17, exact at float32, beyond 65504 between. """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    B, h, w = 2, 96, 160
    scaled = dict(weights50)
    k = np.float32(2.0 ** 17)
    scaled['bn2a_branch2a/gamma'], scaled['bn2a_branch2a/beta'] = scaled['bn2a_branch2a/gamma'] * k, scaled['bn2a_branch2a/beta'] * k
    scaled['res2a_branch2b/kernel'] = scaled['res2a_branch2b/kernel'] / k
    posed = models.load_model(scaled, backbone_name='resnet50', dtype='f16x3', pose=True)
    m32 = models.load_model(scaled, backbone_name='resnet50', dtype='f32', pose=True)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, size=(B, h, w, 3)).astype(np.float32) - MEAN
    inputs = [x, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
    rows, counts = posed.predict_poses_on_batch(inputs, 1.25, (h, w, 3))
    assert posed.range_fallbacks == 1
    want_rows, want_counts = m32.predict_poses_on_batch(inputs, 1.25, (h, w, 3))
    assert same_bytes(rows, want_rows) and same_bytes(counts, want_counts)
    (f_rows, f_counts), _ = posed.predict_poses_on_frames(np.zeros((B, 48, 80, 3), np.uint8), inputs[1], inputs[2])
    assert f_rows.shape == (B, 100, 36) and f_counts.shape == (B,)


def test_run_network_device_pose_writes_the_same_files(tmp_path, monkeypatch):
    """ bin/run_network.py --device-pose against the same run without the flag: the same file set, .mat fields within 1e-4 and KITTI
    fields within 0.011 (the bars of tests/test_harness.py) """
    import scipy.io
    from PIL import Image
    from keras_retinanet_3D.bin import run_network
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    (tmp_path / 'img').mkdir(); (tmp_path / 'calib').mkdir(); (tmp_path / 'host').mkdir(); (tmp_path / 'dev').mkdir()
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    for k in range(3):
        frame = (np.random.default_rng(k).integers(0, 2, size=(375, 1242, 3)) * 255).astype(np.uint8)
        Image.fromarray(frame[:, :, ::-1]).save(str(tmp_path / 'img' / ('%06d.png' % k)))
        (tmp_path / 'calib' / ('%06d.txt' % k)).write_text(calib)
    common = ['synthetic:1234.h5', str(tmp_path / 'img'), str(tmp_path / 'calib'), synthetic.plane_database_path('1k')]
    run_network.main(common + [str(tmp_path / 'host'), '--kitti', '--batch-size', '2'])
    run_network.main(common + [str(tmp_path / 'dev'), '--kitti', '--batch-size', '2', '--device-pose'])

    def tree(root):
        return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, fs in os.walk(str(root)) for f in fs)
    assert tree(tmp_path / 'dev') == tree(tmp_path / 'host') and len(tree(tmp_path / 'dev')) == 6
    for k in range(3):
        a = scipy.io.loadmat(str(tmp_path / 'host' / 'synthetic:1234' / 'outputs' / 'full' / ('%06d.mat' % k)))
        b = scipy.io.loadmat(str(tmp_path / 'dev' / 'synthetic:1234' / 'outputs' / 'full' / ('%06d.mat' % k)))
        assert a['scores'].shape[1] > 0
        for key in ('boxes', 'keypoints', 'labels', 'scores', 'locations', 'angles', 'dimensions', 'residuals'):
            assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, key
            assert np.allclose(a[key], b[key], atol=1e-4), key
        ta = (tmp_path / 'host' / 'synthetic:1234' / 'outputs' / 'kitti' / ('%06d.txt' % k)).read_text().splitlines()
        tb = (tmp_path / 'dev' / 'synthetic:1234' / 'outputs' / 'kitti' / ('%06d.txt' % k)).read_text().splitlines()
        assert len(ta) == len(tb) == a['scores'].shape[1]
        for la, lb in zip(ta, tb):
            fa, fb = la.split(), lb.split()
            assert fa[:3] == fb[:3] == ['Car', '-1', '-1']
            assert np.allclose([float(v) for v in fa[3:]], [float(v) for v in fb[3:]], atol=0.011)
