""" CPU tests of the cuboid NMS: the NumPy form (utils/cuboid_nms.py) against the loop-written oracle
(tests/cuboid_nms_oracle.py) on the issue's cases; what the factoring left of utils.kitti_eval.image_overlaps; the plan with the stage,
built on the CPU device; the option's argument errors; the C ABI's argument checks (host code: they come before any launch); the
command lines. """
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import cuboid_nms_oracle as O
import helpers
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.bin import evaluate_kitti, run_network
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import cuboid_nms as N
from keras_retinanet_3D.utils import kitti_eval

SMALL = O.small_cases()
CLUSTERS = O.cluster_cases()
EXACT = ('exact_at_the_threshold', 'exact_just_below', 'chain', 'equal_scores', 'padding_interleaved', 'all_padding', 'one_row')


def same_as_oracle(rows, metric, threshold, table=None):
    want_rows, want_count, want_by = O.suppress(rows, metric, threshold, table)
    got_rows, got_count, got_by = N.suppress_rows_np(rows, metric, threshold)
    assert got_rows.dtype == np.float32 and got_by.dtype == np.int32
    assert got_count == want_count and got_by.tolist() == want_by
    assert np.array_equal(got_rows.view(np.uint32), want_rows.view(np.uint32))                    # bit for bit, NaN rows included
    return got_rows, got_count, got_by


@pytest.mark.parametrize('name,rows,metric,threshold', SMALL, ids=['{}-{}'.format(c[0], c[2]) for c in SMALL])
def test_host_form_equals_the_oracle(name, rows, metric, threshold):
    table = O.overlap_table(rows, metric)
    if name not in EXACT:
        # what lets the GPU test ask for equality: no overlap so close to the threshold that an ulp of cos / sin could cross it
        assert O.margin(table, threshold) > 1e-9, O.margin(table, threshold)
    out, count, by = same_as_oracle(rows, metric, threshold, table)
    live = rows[:, 14] >= 0
    assert count == int((out[:, 14] >= 0).sum()) and ((by >= 0) == (live & (out[:, 14] < 0))).all()
    kept = by < 0
    assert np.array_equal(out[kept].view(np.uint32), rows[kept].view(np.uint32)) and (out[~kept] == -1).all()


def test_the_cases_say_what_the_issue_says():
    case = {(c[0], c[2]): c for c in SMALL}
    by = lambda name, metric: N.suppress_rows_np(*case[(name, metric)][1:])[2].tolist()  # noqa: E731
    for metric in ('bev', '3d'):
        two = case[('exact_at_the_threshold', metric)][1]
        assert O.overlap(two[0], two[1], metric) == 0.5 and N.pair_overlaps_np(two, metric)[0, 1] == 0.5
        assert by('exact_at_the_threshold', metric) == [-1, -1]          # strict
        assert by('exact_just_below', metric) == [-1, 0]
        assert by('chain', metric) == [-1, 0, -1]                        # B goes and suppresses nothing
        assert by('equal_scores', metric) == [-1, 0, -1, 2]              # the lower row index stays
        assert by('unsorted', metric) == [3, -1, 3, -1, 1, -1]           # the rank is the score's, not the row's
        assert by('nan_row_between', metric) == [-1, -1, 0]              # the NaN row stays; the duplicates do not see it
        assert by('padding_interleaved', metric) == [-1, -1, -1, -1, 1, -1, -1, -1, -1, -1]
        assert by('all_padding', metric) == [-1] * 5 and by('one_row', metric) == [-1]
        assert N.suppress_rows_np(*case[('d128', metric)][1:])[1] == 32
    assert by('bridge', 'bev') == [-1, 0] and by('bridge', '3d') == [-1, -1]


@pytest.mark.parametrize('name,rows,metric,threshold', CLUSTERS, ids=['{}-{}'.format(c[0], c[2]) for c in CLUSTERS])
def test_clusters_equal_the_oracle(name, rows, metric, threshold):
    """ case (viii): exact under its condition -- no oracle overlap within 1e-6 of the threshold -- which is asserted here """
    assert rows.shape == (40, 36)
    table = O.overlap_table(rows, metric)
    assert O.margin(table, threshold) > 1e-6
    _, count, by = same_as_oracle(rows, metric, threshold, table)
    assert 10 <= count < 40
    over = N.pair_overlaps_np(rows, metric)
    assert max(abs(over[i, j] - o) for (i, j), o in table.items()) <= 1e-12 and np.array_equal(over, over.T)


def test_image_overlaps_still_returns_what_it_returned():
    """ the factoring moved the clipping into a function: a detection against itself is 1, and the pair table is image_overlaps' plane """
    rows = CLUSTERS[0][1]
    labels = np.zeros((rows.shape[0], 16))
    labels[:, 8], labels[:, 9], labels[:, 10] = rows[:, 30], rows[:, 17], rows[:, 18]
    labels[:, 11], labels[:, 12], labels[:, 13], labels[:, 14] = rows[:, 19], rows[:, 31], rows[:, 21], rows[:, 32]
    planes = kitti_eval.image_overlaps(rows, labels)
    assert np.allclose(np.diag(planes[1]), 1.0, atol=1e-12) and np.allclose(np.diag(planes[2]), 1.0, atol=1e-12)
    for code, metric in ((1, 'bev'), (2, '3d')):
        pair = N.pair_overlaps_np(rows, metric)
        upper = np.triu_indices(rows.shape[0], 1)
        assert np.array_equal(planes[code][upper], pair[upper])


# ---------------------------------------------------------------------------------------------------- the plan
@pytest.fixture(scope='module')
def cpu_models():
    """ (pose=True, pose=True + cuboid_nms) models on the CPU device, as tests/test_pose_cpu.py builds them """
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')
        weights = W.synthetic_weights('resnet50', 1234)
        yield {dt: (models.load_model(weights, backbone_name='resnet50', dtype=dt, pose=True),
                    models.load_model(weights, backbone_name='resnet50', dtype=dt, pose=True, cuboid_nms=('3d', 0.25)))
               for dt in ('f16x3', 'f32')}


PLAN_CASES = [(dt, env, B) for dt, B in (('f16x3', 8), ('f32', 2)) for env in (helpers.PLAN_OPTIONS[0], helpers.PLAN_OPTIONS[10])]


@pytest.mark.parametrize('dt,env,B', PLAN_CASES, ids=['{} B={} {}'.format(dt, B, sorted(env.items())) for dt, env, B in PLAN_CASES])
def test_cuboid_nms_plan_is_the_pose_plan_plus_one_trailing_op(dt, env, B, cpu_models, monkeypatch):
    posed, suppressed = cpu_models[dt]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plans = []
    for m in (posed, suppressed):
        m._plans.clear()
        plans.append(m.plan_for(B, 200, 333, 100, True))
        m._plans.clear()
    a, b = plans
    assert len(b.ops) == len(a.ops) + 1
    head = lambda p, n: [(kind, tag, name, flops, lane) for (kind, tag, _, name, flops), lane in zip(p.ops[:n], p.lanes[:n])]  # noqa: E731
    assert head(b, len(a.ops)) == head(a, len(a.ops))
    assert [b.array[i].kind for i in range(len(a.ops))] == [a.array[i].kind for i in range(len(a.ops))]
    kind, tag, desc, name, flops = b.ops[-1]
    assert (kind, tag, name, b.lanes[-1]) == (R.OP_CUBOID_NMS, 0, 'suppress_cuboids', 0) and a.ops[-1][0] == R.OP_POSE == b.ops[-2][0]
    assert R.OP_CUBOID_NMS == 20 and b.array[len(b.ops) - 1].kind == R.OP_CUBOID_NMS | (10 << 20)      # lane 0, no join, stage 10 ("gpp:cuboid_nms")
    assert (desc.B, desc.D, desc.metric, desc.reserved, desc.iou_thr) == (B, 100, 1, 0, 0.25)
    assert desc.rows == b.pose_rows.data_ptr() and desc.counts == b.pose_counts.data_ptr() and desc.suppressor == b.pose_suppressor.data_ptr()
    assert tuple(b.pose_suppressor.shape) == (B, 100) and b.pose_suppressor.dtype == torch.int32 and not hasattr(a, 'pose_suppressor')
    assert b.tagged == a.tagged and b.flops == a.flops
    assert a.check_stream_ordering() == [] and b.check_stream_ordering() == []
    reads, writes = b.access[-1]
    assert set(R.Plan.spans([b.pose_rows])) == set(reads)
    assert set(R.Plan.spans([b.pose_rows, b.pose_counts, b.pose_suppressor])) == set(writes)
    # the pose op in front of it is what it was
    pose = b.ops[-2][2]
    assert pose.rows == b.pose_rows.data_ptr() and pose.counts == b.pose_counts.data_ptr() and abs(pose.score_thr - 0.05) < 1e-9


def test_descriptor_mirrors_the_header():
    assert ctypes.sizeof(R.CuboidNmsDesc) == 48 and R.CuboidNmsDesc.iou_thr.offset == 24 and R.CuboidNmsDesc.B.offset == 32
    text = open(os.path.join(helpers.ROOT, 'include', 'gpp.h')).read()
    assert '#define GPP_OP_CUBOID_NMS 20' in text and '#define GPP_CUBOID_NMS_BEV 0' in text and '#define GPP_CUBOID_NMS_3D 1' in text
    assert N.METRICS == ('bev', '3d')


def test_option_errors(cpu_models):
    weights = W.synthetic_weights('resnet50', 1234)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        with pytest.raises(ValueError, match='pose=True'):
            models.load_model(weights, backbone_name='resnet50', dtype='f32', cuboid_nms=('bev', 0.3))
        for bad in (('side', 0.3), ('bev', 0.0), ('bev', 1.0), ('3d', float('nan')), 'bev', ('bev',)):
            with pytest.raises(ValueError):
                models.load_model(weights, backbone_name='resnet50', dtype='f32', pose=True, cuboid_nms=bad)
    posed, suppressed = cpu_models['f32']
    assert posed.cuboid_nms is None and suppressed.cuboid_nms == ('3d', 0.25)
    with pytest.raises(hip.GppError):
        posed.cuboid_suppressors()
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            N.suppress_rows_np(SMALL[0][1], 'bev', bad)
    with pytest.raises(ValueError):
        N.suppress_rows_np(SMALL[0][1], 'image', 0.5)


def test_c_abi_argument_checks():
    """ every one of them returns before a launch: they run without a GPU """
    lib = hip.lib()
    buf = (ctypes.c_float * (2 * 129 * 36))()
    ints = (ctypes.c_int32 * (2 * 129))()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ints, ctypes.c_void_p)
    call = lambda rows, B, D, metric, thr, out, counts, by: lib.gpp_cuboid_nms_f64(rows, B, D, metric, thr, out, counts, by, None)  # noqa: E731
    assert call(p, 1, 129, 0, 0.5, p, q, q) == -4                                                  # GPP_ERR_UNSUPPORTED
    for args in ((None, 1, 4, 0, 0.5, p, q, q), (p, 1, 4, 0, 0.5, None, q, q), (p, 1, 4, 0, 0.5, p, None, q), (p, 1, 4, 0, 0.5, p, q, None),
                 (p, -1, 4, 0, 0.5, p, q, q), (p, 1, -4, 0, 0.5, p, q, q), (p, 1, 4, 2, 0.5, p, q, q), (p, 1, 4, -1, 0.5, p, q, q),
                 (p, 1, 4, 0, 0.0, p, q, q), (p, 1, 4, 0, 1.0, p, q, q), (p, 1, 4, 0, float('nan'), p, q, q), (p, 0, 4, 7, 0.5, p, q, q)):
        assert call(*args) == -1, args                                                             # GPP_ERR_BAD_ARG
    assert call(p, 0, 4, 0, 0.5, p, q, q) == 0 and call(p, 3, 0, 1, 0.5, p, q, q) == 0 and call(None, 0, 0, 0, 0.5, None, None, None) == 0
    # the plan runner refuses a descriptor with a non-zero reserved word before anything is launched
    desc = R.CuboidNmsDesc(p.value, q.value, q.value, 0.5, 1, 4, 0, 1)
    op = R.PlanOp(R.OP_CUBOID_NMS, 0, ctypes.addressof(desc))
    assert lib.gpp_plan_run(ctypes.byref(op), 1, None, None, 0) == -1


# ---------------------------------------------------------------------------------------------------- the command lines
def kitti_line(g, score=None):
    return 'Car {:.2f} {:d} '.format(g[1], int(g[2])) + ' '.join('%.2f' % v for v in g[3:15]) + ('' if score is None else ' %.2f' % score) + '\n'


def test_evaluate_kitti_cuboid_nms_removes_the_duplicate(tmp_path, capsys):
    """ three labelled Cars, each detected exactly; one detected a second time 0.25 m to the side with an image box that overlaps the first
    by less than 0.5 (the decode's NMS keeps such a pair): a false positive, which the suppression removes -- the true positives stay """
    cars = [np.array([0, 0.0, 0, -1.5, 100.0 + 200 * k, 150.0, 220.0 + 200 * k, 230.0, 1.5, 1.6, 4.0, -6.0 + 6.0 * k, 1.65, 20.0 + 3 * k, -1.5 + 0.1 * k, 0])
            for k in range(3)]
    label_dir, result_dir = tmp_path / 'label_2', tmp_path / 'results'
    label_dir.mkdir(), result_dir.mkdir()
    (label_dir / '000000.txt').write_text(''.join(kitti_line(g) for g in cars))
    twin = cars[1].copy()
    twin[4:8] = (340.0, 150.0, 420.0, 230.0)                             # image IoU with its original: 80 / 160 = 0.5 -- not above 0.5
    twin[11] += 0.25
    (result_dir / '000000.txt').write_text(''.join(kitti_line(g, 0.9 - 0.1 * k) for k, g in enumerate(cars)) + kitti_line(twin, 0.75))
    plain = evaluate_kitti.main([str(label_dir), str(result_dir), '--json', str(tmp_path / 'a.json')])
    nms = evaluate_kitti.main([str(label_dir), str(result_dir), '--cuboid-nms', 'bev', '--cuboid-nms-threshold', '0.5', '--json', str(tmp_path / 'b.json')])
    capsys.readouterr()
    for metric in kitti_eval.METRICS:
        for difficulty in kitti_eval.DIFFICULTIES:
            a, b = plain[(metric, difficulty)], nms[(metric, difficulty)]
            assert a['tp'].tolist() == b['tp'].tolist() == [1, 2, 3] and a['fn'].tolist() == b['fn'].tolist()
            assert a['fp'].tolist() == [0, 0, 1] and b['fp'].tolist() == [0, 0, 0], (metric, difficulty)
            assert b['ap_r40'] > a['ap_r40']
    for argv in (['--cuboid-nms', 'bev'], ['--cuboid-nms-threshold', '0.5'], ['--cuboid-nms', 'bev', '--cuboid-nms-threshold', '1.0'],
                 ['--cuboid-nms', 'side', '--cuboid-nms-threshold', '0.5']):
        with pytest.raises(SystemExit):
            evaluate_kitti.parse_args([str(label_dir), str(result_dir)] + argv)
    capsys.readouterr()


def test_run_network_flags_go_together(capsys):
    base = ['synthetic:1', 'images', 'calib', 'planes.mat', 'out']
    args = run_network.parse_args(base + ['--cuboid-nms', '3d', '--cuboid-nms-threshold', '0.25'])
    assert (args.cuboid_nms, args.cuboid_nms_threshold) == ('3d', 0.25)
    assert run_network.parse_args(base).cuboid_nms is None
    for argv in (['--cuboid-nms', 'bev'], ['--cuboid-nms-threshold', '0.3'], ['--cuboid-nms', 'bev', '--cuboid-nms-threshold', '0']):
        with pytest.raises(SystemExit):
            run_network.parse_args(base + argv)
    capsys.readouterr()


def test_host_path_suppression_of_a_detection_dict():
    """ bin/run_network.py without --device-pose: the dict of recover_pose loses the duplicate, every array alike """
    n = 3
    det = {'boxes': np.zeros((n, 12), np.float32), 'scores': np.array([0.9, 0.8, 0.7], np.float32), 'labels': np.zeros(n, np.int32),
           'orientations': np.zeros(n, np.int32), 'residuals': np.zeros(n, np.float32), 'keypoints': np.zeros((n, 12), np.float32),
           'dimensions': np.tile(np.array([1.5, 1.6, 4.0], np.float32), (n, 1)),
           'locations': np.array([[0.0, 1.65, 20.0], [0.25, 1.65, 20.0], [8.0, 1.65, 20.0]], np.float32),
           'angles': np.array([[0.0, 0.3, 0.0]] * n, np.float32)}
    out, by = N.suppress_detections(det, 'bev', 0.5)
    assert by.tolist() == [-1, 0, -1] and out['scores'].tolist() == pytest.approx([0.9, 0.7])
    assert all(len(out[k]) == 2 for k in det) and np.array_equal(out['locations'], det['locations'][[0, 2]])
    rows = np.concatenate([O.padding(1), SMALL[2][1], O.padding(1)])
    first = N.live_first(N.suppress_rows_np(rows, 'bev', 0.4)[0])
    assert (first[:2, 14] >= 0).all() and (first[2:] == -1).all() and first[:2, 12].tolist() == pytest.approx([0.9, 0.7])
    assert math.isclose(float(first[1, 19]), 2.0)
