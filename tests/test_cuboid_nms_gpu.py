""" GPU tests of the cuboid NMS (csrc/cuboid_nms.hip): the kernel against the NumPy form (utils/cuboid_nms.py)
and the loop-written oracle (tests/cuboid_nms_oracle.py) on the cases of tests/test_cuboid_nms_cpu.py; in place and out of place; the
C ABI chain label_prep -> poll -> pose -> cuboid NMS -> KITTI; RetinaNet3D(pose=True, cuboid_nms=...) end to end; bin/run_network.py. """
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import cuboid_nms_oracle as O
import label_prep_oracle as LO
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import cuboid_nms as N
from keras_retinanet_3D.utils import gpp_utils, kitti_eval, synthetic
from keras_retinanet_3D.utils import label_prep as L

pytestmark = pytest.mark.gpu

SMALL = O.small_cases()
CLUSTERS = O.cluster_cases()
MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_run(rows, metric, threshold):
    out, counts, by = N.suppress_rows_device(np.asarray(rows, np.float32)[None], metric, threshold)
    assert out.shape == (1,) + rows.shape and out.dtype == np.float32 and counts.dtype == np.int32 and by.dtype == np.int32
    return out[0], int(counts[0]), by[0]


@pytest.mark.parametrize('name,rows,metric,threshold', SMALL, ids=['{}-{}'.format(c[0], c[2]) for c in SMALL])
def test_kernel_equals_the_host_form(name, rows, metric, threshold):
    """ cases (i) - (vii): exactly.  r_y = 0 with dyadic sizes, or margins of more than 1e-9 (asserted by tests/test_cuboid_nms_cpu.py) """
    want_rows, want_count, want_by = N.suppress_rows_np(rows, metric, threshold)
    got_rows, got_count, got_by = device_run(rows, metric, threshold)
    assert got_count == want_count and got_by.tolist() == want_by.tolist()
    assert same_bytes(got_rows, want_rows)


@pytest.mark.parametrize('name,rows,metric,threshold', CLUSTERS, ids=['{}-{}'.format(c[0], c[2]) for c in CLUSTERS])
def test_kernel_decides_as_the_oracle_on_the_clusters(name, rows, metric, threshold):
    """ case (viii): no oracle overlap lies within 1e-6 of the threshold, so the decisions are the oracle's """
    table = O.overlap_table(rows, metric)
    assert O.margin(table, threshold) > 1e-6
    want_rows, want_count, want_by = O.suppress(rows, metric, threshold, table)
    got_rows, got_count, got_by = device_run(rows, metric, threshold)
    assert got_count == want_count and got_by.tolist() == want_by and same_bytes(got_rows, want_rows)


def batch_of_three():
    """ B = 3, D = 40: ten clusters of four, a chain among padding, nothing """
    chain = [c for c in SMALL if c[0] == 'padding_interleaved'][0][1]
    return np.stack([CLUSTERS[0][1], np.concatenate([chain, O.padding(40 - chain.shape[0])]), O.padding(40)])


@pytest.mark.parametrize('metric', ['bev', '3d'])
def test_batch_in_place_out_of_place_and_twice(metric):
    rows = batch_of_three()
    want = N.suppress_batch_np(rows, metric, O.CLUSTER_THRESHOLD)
    assert want[1].tolist()[1:] == [2, 0] and 10 <= want[1][0] < 40
    code = N.metric_code(metric)
    src = torch.as_tensor(rows).cuda()
    out, counts, by = hip.cuboid_nms(src, code, O.CLUSTER_THRESHOLD)
    assert same_bytes(src.cpu().numpy(), rows)                                   # out of place: the input is left alone
    got = (out.cpu().numpy(), counts.cpu().numpy(), by.cpu().numpy())
    for g, w in zip(got, want):
        assert same_bytes(g, w)
    again = hip.cuboid_nms(src, code, O.CLUSTER_THRESHOLD)
    for g, a in zip(got, again):
        assert same_bytes(g, a.cpu().numpy())
    work = src.clone()
    out2, counts2, by2 = hip.cuboid_nms(work, code, O.CLUSTER_THRESHOLD, out=work)
    assert out2 is work
    for g, a in zip(got, (work, counts2, by2)):
        assert same_bytes(g, a.cpu().numpy())
    # the suppressed set is a fixed point: a second pass over its own result removes nothing
    out3, counts3, by3 = hip.cuboid_nms(work, code, O.CLUSTER_THRESHOLD, out=work)
    assert same_bytes(out3.cpu().numpy(), got[0]) and same_bytes(counts3.cpu().numpy(), got[1]) and (by3.cpu().numpy() == -1).all()


def test_bad_arguments_launch_nothing():
    lib = hip.lib()
    rows = torch.as_tensor(batch_of_three()).cuda()
    before = rows.cpu().numpy()
    counts = torch.full((3,), 77, dtype=torch.int32, device='cuda')
    by = torch.full((3, 129), 77, dtype=torch.int32, device='cuda')
    p, c, s = hip.ptr(rows), hip.ptr(counts), hip.ptr(by)
    call = lambda rows_in, B, D, metric, thr, out, cnt, sup: lib.gpp_cuboid_nms_f64(rows_in, B, D, metric, thr, out, cnt, sup, hip.stream_ptr())  # noqa: E731
    assert call(p, 1, 129, 0, 0.3, p, c, s) == -4
    for args in ((None, 3, 40, 0, 0.3, p, c, s), (p, 3, 40, 0, 0.3, None, c, s), (p, 3, 40, 0, 0.3, p, None, s), (p, 3, 40, 0, 0.3, p, c, None),
                 (p, 3, 40, 2, 0.3, p, c, s), (p, 3, 40, 0, 0.0, p, c, s), (p, 3, 40, 0, 1.0, p, c, s), (p, -3, 40, 0, 0.3, p, c, s)):
        assert call(*args) == -1, args
    assert call(p, 0, 40, 0, 0.3, p, c, s) == 0 and call(p, 3, 0, 1, 0.3, p, c, s) == 0
    torch.cuda.synchronize()
    assert same_bytes(rows.cpu().numpy(), before) and (counts.cpu().numpy() == 77).all() and (by.cpu().numpy() == 77).all()
    with pytest.raises(hip.GppError):
        hip.cuboid_nms(torch.zeros((1, 129, 36), dtype=torch.float32, device='cuda'), 0, 0.3)
    empty = hip.cuboid_nms(torch.zeros((0, 40, 36), dtype=torch.float32, device='cuda'), 0, 0.3)
    assert tuple(empty[0].shape) == (0, 40, 36) and tuple(empty[1].shape) == (0,)


# ---------------------------------------------------------------------------------------------------- the chain through the C ABI
P_CAM = np.array([[721.5377, 0.0, 609.5593, 0.0], [0.0, 721.5377, 172.854, 0.0], [0.0, 0.0, 1.0, 0.0]])
T_Y = 1.65


def six_cars(seed):
    """ six Cars on the plane y = 1.65 between 12 and 38 m, every one high enough for Moderate, their own projected box as the label box """
    rng = np.random.default_rng(seed)
    cars = []
    for k in range(6):
        z, x = 12.0 + 5.0 * k + rng.uniform(-1.0, 1.0), -8.0 + 3.2 * k + rng.uniform(-0.5, 0.5)
        ry = rng.uniform(-math.pi, math.pi)
        alpha = (ry - math.atan2(x, z) + math.pi) % (2 * math.pi) - math.pi
        cars.append(LO.make_label(0, 0.0, 0, alpha, (0.0, 0.0, 0.0, 0.0), (1.5, 1.6, 4.0), (x, T_Y, z), ry))
    cars = np.array(cars)
    cars[:, 4:8] = L.prepare(cars, P_CAM)[:, 4:8]
    return cars


def with_twins(cars):
    """ every Car a second time: 0.25 m to the side, in the neighbouring orientation class (alpha a quarter turn on) """
    twins = cars.copy()
    twins[:, 11] += 0.25
    twins[:, 3] = (twins[:, 3] + math.pi / 2 + math.pi) % (2 * math.pi) - math.pi
    twins[:, 4:8] = L.prepare(twins, P_CAM)[:, 4:8]
    return np.concatenate([cars, twins])


def test_chain_label_prep_poll_pose_nms_kitti():
    """ two images of six labelled Cars, each detected twice (the second copy with score 0.5): without the stage the copies are twelve
    false positives at Moderate, with it ('bev', 0.5) none -- and the true positives are the same detections """
    dev = hip.require_device()
    truth = [six_cars(31), six_cars(32)]
    seen = [with_twins(g) for g in truth]
    B, D = 2, 12
    labels_d, counts_d, P_d, trig_d = L._upload(seen, [P_CAM] * B, D, dev)
    _, (boxes, dims, scores, det_labels, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, L.CAR, True, True)
    o = orient.cpu().numpy()
    assert (o >= 0).all() and ((o[:, 6:] - o[:, :6]) != 0).all()                # the copies sit in another orientation class
    scores[:, 6:] = 0.5
    planes_d = torch.as_tensor(np.array([[0.0, -1.0, 0.0, T_Y], [0.0, -1.0, 0.0, T_Y + 0.4]], np.float32)).to(dev)
    pinv_d = torch.as_tensor(np.tile(np.linalg.pinv(P_CAM).astype(np.float32), (B, 1, 1))).to(dev)
    info_d = torch.as_tensor(np.array([[1.0, 376.0, 1242.0]] * B, np.float32)).to(dev)
    keypoints, _, residuals = gpp_utils.fit_road_planes(boxes, dims, orient, pinv_d, planes_d)
    rows = torch.empty((B, D, hip.GPP_POSE_COLS), dtype=torch.float32, device=dev)
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    hip.check(hip.lib().gpp_pose_f32(hip.ptr(boxes), hip.ptr(dims), hip.ptr(scores), hip.ptr(det_labels), hip.ptr(orient), hip.ptr(keypoints),
                                     hip.ptr(residuals), hip.ptr(info_d), B, D, gpp_utils.POSE_SCORE_THRESHOLD, hip.ptr(rows), hip.ptr(counts),
                                     hip.stream_ptr()), 'gpp_pose_f32')
    assert counts.cpu().numpy().tolist() == [12, 12]
    kept_rows, kept_counts, by = hip.cuboid_nms(rows, N.metric_code('bev'), 0.5)
    assert kept_counts.cpu().numpy().tolist() == [6, 6]
    assert by.cpu().numpy().tolist() == [[-1] * 6 + list(range(6))] * 2          # copy k + 6 went, removed by car k
    want = N.suppress_batch_np(rows.cpu().numpy(), 'bev', 0.5)
    assert same_bytes(kept_rows.cpu().numpy(), want[0]) and same_bytes(by.cpu().numpy(), want[2])

    packed, label_counts = kitti_eval.pack_labels(truth, 6)
    gt_d, gt_counts_d = torch.as_tensor(packed).to(dev), torch.as_tensor(label_counts).to(dev)
    thresholds = torch.zeros((3, 3, 1), dtype=torch.float32, device=dev)          # every detection is in
    n_thresholds = torch.ones((3, 3), dtype=torch.int32, device=dev)
    stats = {}
    for name, r in (('plain', rows), ('nms', kept_rows)):
        overlaps = hip.kitti_overlaps(r, gt_d, gt_counts_d)
        s, _ = hip.kitti_stats(r, gt_d, gt_counts_d, overlaps, (0.7, 0.7, 0.7), thresholds, n_thresholds)
        tp, _ = hip.kitti_stats(r, gt_d, gt_counts_d, overlaps, (0.7, 0.7, 0.7))
        stats[name] = (s.cpu().numpy()[:, :, :, 0, :].sum(axis=0), tp.cpu().numpy())          # (metric, difficulty, tp fp fn)
    print('tp fp fn per (metric, difficulty) without the stage:', stats['plain'][0].tolist(), 'with it:', stats['nms'][0].tolist())
    for metric in range(3):
        assert stats['plain'][0][metric, 1].tolist() == [12, 12, 0]
        assert stats['nms'][0][metric, 1].tolist() == [12, 0, 0]
        assert stats['nms'][0][metric, :, 1].tolist() == [0, 0, 0]
    assert same_bytes(stats['plain'][1], stats['nms'][1])                       # the same true positives, label by label


# ---------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope='module')
def weights50():
    return W.synthetic_weights('resnet50', 1234)


def test_model_rows_are_the_suppressed_rows_of_the_plain_pose_model(weights50, monkeypatch):
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    B, h, w = 2, 200, 333
    rng = np.random.default_rng(200)
    frames = (rng.integers(0, 2, size=(B, h, w, 3)) * 255).astype(np.float32) - MEAN
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    inputs = [frames, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
    scale, shape = 1.0, (h, w, 3)
    posed = models.load_model(weights50, backbone_name='resnet50', dtype='f16x3', pose=True)
    rows, counts = posed.predict_poses_on_batch(inputs, scale, shape)
    assert counts.sum() > 0
    usable = []
    for t in (0.25, 0.3, 0.35, 0.4):
        over = np.stack([N.pair_overlaps_np(r, 'bev') for r in rows])
        with np.errstate(invalid='ignore'):
            if not (np.abs(over - t) <= 1e-6).any():
                usable.append(t)
    assert usable, 'every candidate threshold has a host-form overlap within 1e-6 of it'
    t = usable[0]
    model = models.load_model(weights50, backbone_name='resnet50', dtype='f16x3', pose=True, cuboid_nms=('bev', t))
    got_rows, got_counts = model.predict_poses_on_batch(inputs, scale, shape)
    want_rows, want_counts, want_by = N.suppress_batch_np(rows, 'bev', t)
    print('threshold {}: {} rows, {} kept'.format(t, counts.tolist(), want_counts.tolist()))
    assert same_bytes(got_rows, want_rows) and same_bytes(got_counts, want_counts)
    assert same_bytes(model.cuboid_suppressors(), want_by)
    for a, b in zip(model.predict_on_batch(inputs), posed.predict_on_batch(inputs)):
        assert same_bytes(a, b)
    assert model.range_fallbacks == 0 and posed.range_fallbacks == 0
    with pytest.raises(hip.GppError):
        posed.cuboid_suppressors()


def test_run_network_device_pose_cuboid_nms_drops_the_named_lines(tmp_path, monkeypatch):
    """ bin/run_network.py --device-pose --cuboid-nms bev --cuboid-nms-threshold 0.3 on three small frames: its KITTI files are those of
    the run without the two flags minus exactly the lines that cuboid_suppressors() names """
    from PIL import Image
    from keras_retinanet_3D.bin import run_network
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    (tmp_path / 'img').mkdir(); (tmp_path / 'calib').mkdir(); (tmp_path / 'plain').mkdir(); (tmp_path / 'nms').mkdir()
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    for k in range(3):
        frame = (np.random.default_rng(k).integers(0, 2, size=(402, 640, 3)) * 255).astype(np.uint8)      # (scale 1: the noise survives the resize)
        Image.fromarray(frame[:, :, ::-1]).save(str(tmp_path / 'img' / ('%06d.png' % k)))
        (tmp_path / 'calib' / ('%06d.txt' % k)).write_text(calib)
    tables = []
    load = models.load_model

    def load_and_watch(*args, **kwargs):
        model = load(*args, **kwargs)
        if model.cuboid_nms is not None:
            call = model.predict_poses_on_frames

            def watched(*a, **k):
                result = call(*a, **k)
                tables.append(model.cuboid_suppressors())
                return result
            model.predict_poses_on_frames = watched
        return model
    monkeypatch.setattr(run_network.models, 'load_model', load_and_watch)
    common = ['synthetic:1234.h5', str(tmp_path / 'img'), str(tmp_path / 'calib'), synthetic.plane_database_path('100')]
    run_network.main(common + [str(tmp_path / 'plain'), '--kitti', '--batch-size', '3', '--device-pose'])
    assert tables == []
    run_network.main(common + [str(tmp_path / 'nms'), '--kitti', '--batch-size', '3', '--device-pose', '--cuboid-nms', 'bev', '--cuboid-nms-threshold', '0.3'])
    assert len(tables) == 1 and tables[0].shape == (3, 100)
    files = os.listdir(str(tmp_path / 'calib'))                                  # (the order run_network reads them in: one call of three)
    removed = 0
    for b, f in enumerate(files):
        plain = (tmp_path / 'plain' / 'synthetic:1234' / 'outputs' / 'kitti' / f).read_text().splitlines()
        nms = (tmp_path / 'nms' / 'synthetic:1234' / 'outputs' / 'kitti' / f).read_text().splitlines()
        assert len(plain) > 0 and (tables[0][b, len(plain):] == -1).all()
        assert nms == [line for d, line in enumerate(plain) if tables[0][b, d] < 0]
        removed += len(plain) - len(nms)
    print('lines removed by the stage:', removed)
