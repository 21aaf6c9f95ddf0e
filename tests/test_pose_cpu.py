""" CPU tests of the device pose stage (csrc/pose.hip, RetinaNet3D(pose=True)): the float64 oracle the GPU tests measure against
(tests/pose_oracle.py) reproduces the reference's own run_network outputs; the row readers of utils.gpp_utils; the C ABI's argument
checks (host code: they come before any launch); the plan with and without the stage, built on the CPU device. """
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import helpers
import pose_oracle as O
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import gpp_utils

CASES = sorted(glob.glob(os.path.join(helpers.GOLDEN, 'harness_*.npz')))


@pytest.mark.parametrize('path', CASES, ids=[os.path.basename(p) for p in CASES])
def test_oracle_reproduces_the_reference_harness(path):
    """ the bars of tests/test_harness.py: 1e-4 on the .mat fields, 0.011 on the KITTI text fields """
    g = dict(np.load(path))
    outs, scales, shapes = O.fixture_outputs(os.path.basename(path))
    rows, counts = O.pose_rows(outs, scales, shapes)
    n = g['mat_scores'].shape[1]
    assert counts.tolist() == [n]
    r = rows[0, :n]
    assert (rows[0, n:] == -1).all()
    assert np.allclose(r[:, O.BOX], g['mat_boxes'], atol=1e-4) and np.allclose(r[:, O.KP2D], g['mat_keypoints'], atol=1e-4)
    assert np.array_equal(r[:, O.LABEL], g['mat_labels'][0]) and np.allclose(r[:, O.SCORE], g['mat_scores'][0])
    assert np.allclose(r[:, O.DIMS], g['mat_dimensions'], atol=1e-4)
    assert np.allclose(r[:, O.LOC], g['mat_locations'], atol=1e-4)
    assert np.allclose(r[:, O.ROT], g['mat_angles'], atol=1e-4)
    assert np.allclose(r[:, O.RESIDUAL], g['mat_residuals'][0], atol=1e-6)
    want = str(g['kitti_text']).splitlines()
    lines = O.kitti_lines(rows[0], n)
    assert len(lines) == len(want)
    for a, b in zip(lines, want):
        fa, fb = a.split(), b.split()
        assert fa[:3] == fb[:3] == ['Car', '-1', '-1']
        assert np.allclose([float(v) for v in fa[3:]], [float(v) for v in fb[3:]], atol=0.011)


def test_oracle_rows_of_the_fixtures_are_regular():
    """ what the GPU comparison relies on: no degenerate row, every row above the threshold, counted rows a prefix """
    outs, scales, shapes = O.fixture_outputs('fullsize_resnet50_1k_s2024_f64.npz')
    rows, counts = O.pose_rows(outs, scales, shapes)
    assert counts.tolist() == [100] * 8 and np.isfinite(rows).all() and (rows[..., 33:] == 0).all()
    assert (np.abs(rows[..., O.ALPHA]) <= np.pi).all() and (np.abs(rows[..., O.R_Y]) <= np.pi).all()


def test_kitti_text_from_rows_equals_the_per_row_loop():
    outs, scales, shapes = O.fixture_outputs('harness_000007.npz')
    rows, counts = O.pose_rows(outs, scales, shapes)
    rows32 = rows.astype(np.float32)
    n = int(counts[0])
    loop = ''.join(gpp_utils.KITTI_FORMAT % tuple(rows32[0, i, c] for c in gpp_utils.KITTI_COLUMNS) for i in range(n))
    text = gpp_utils.kitti_lines_from_rows(rows32[0], n)
    assert text == loop and text.count('\n') == n and n > 0
    assert text == ''.join(O.kitti_lines(rows32[0], n))                 # the oracle's own column order
    assert gpp_utils.kitti_lines_from_rows(rows32[0], 0) == ''
    det = gpp_utils.detections_from_rows(rows32[0], n)
    host = gpp_utils.recover_pose(gpp_utils.select_detections(outs, scales[0]))
    for key in ('boxes', 'dimensions', 'scores', 'labels', 'orientations', 'residuals', 'locations', 'angles'):
        assert det[key].dtype == host[key].dtype and det[key].shape == host[key].shape, key
        assert np.allclose(det[key], host[key], atol=1e-4), key
    for key in ('alpha', 'kitti_h', 'kitti_y', 'r_y'):
        assert det[key].shape == (n,) and det[key].dtype == np.float32
    assert det['kitti_box'].shape == (n, 4)


def test_abi_exports_pose_and_checks_arguments_before_any_launch():
    lib = hip.lib()
    assert hasattr(lib, 'gpp_pose_f32')
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = [p] * 8
    assert lib.gpp_pose_f32(*(ok + [-1, 4, 0.05, p, p, None])) == -1           # GPP_ERR_BAD_ARG
    assert lib.gpp_pose_f32(*(ok + [1, -4, 0.05, p, p, None])) == -1
    for k in range(8):
        args = list(ok)
        args[k] = None
        assert lib.gpp_pose_f32(*(args + [1, 1, 0.05, p, p, None])) == -1, k
    assert lib.gpp_pose_f32(*(ok + [1, 1, 0.05, None, p, None])) == -1
    assert lib.gpp_pose_f32(*(ok + [1, 1, 0.05, p, None, None])) == -1
    assert lib.gpp_pose_f32(*(ok + [0, 100, 0.05, p, p, None])) == 0           # nothing to do: GPP_OK, nothing launched
    assert lib.gpp_pose_f32(*(ok + [8, 0, 0.05, p, p, None])) == 0


def test_pose_fails_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    outs, scales, shapes = O.fixture_outputs('harness_000007.npz')
    with pytest.raises(hip.GppError):
        gpp_utils.recover_pose_device(outs, scales, shapes)


@pytest.fixture(scope='module')
def cpu_models():
    """ (pose=False, pose=True) models on the CPU device, as tests/test_plan_cpu.py builds them """
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')
        weights = W.synthetic_weights('resnet50', 1234)
        yield {dt: (models.load_model(weights, backbone_name='resnet50', dtype=dt), models.load_model(weights, backbone_name='resnet50', dtype=dt, pose=True))
               for dt in ('f16x3', 'f32')}


PLAN_CASES = [(dt, env, B) for dt, B in (('f16x3', 8), ('f32', 2), ('f16x3', 1))
              for env in (helpers.PLAN_OPTIONS[0], helpers.PLAN_OPTIONS[6], helpers.PLAN_OPTIONS[10], helpers.PLAN_OPTIONS[11], helpers.PLAN_OPTIONS[15])]


@pytest.mark.parametrize('dt,env,B', PLAN_CASES, ids=['{} B={} {}'.format(dt, B, sorted(env.items())) for dt, env, B in PLAN_CASES])
def test_pose_plan_is_the_plain_plan_plus_one_trailing_op(dt, env, B, cpu_models, monkeypatch):
    plain, posed = cpu_models[dt]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plans = []
    for m in (plain, posed):
        m._plans.clear()
        plans.append(m.plan_for(B, 200, 333, 100, True))
        m._plans.clear()
    a, b = plans
    assert len(b.ops) == len(a.ops) + 1
    head = lambda p, n: [(kind, tag, name, flops, lane) for (kind, tag, _, name, flops), lane in zip(p.ops[:n], p.lanes[:n])]  # noqa: E731
    assert head(b, len(a.ops)) == head(a, len(a.ops))
    assert [b.array[i].kind for i in range(len(a.ops))] == [a.array[i].kind for i in range(len(a.ops))]
    kind, tag, desc, name, flops = b.ops[-1]
    assert (kind, tag, name, b.lanes[-1]) == (R.OP_POSE, 0, 'recover_pose', 0) and a.ops[-1][0] == R.OP_POLL
    assert b.array[len(b.ops) - 1].kind == R.OP_POSE | (8 << 20)           # lane 0, no join flag, stage 8 ("gpp:pose")
    assert (desc.B, desc.D) == (B, 100) and abs(desc.score_thr - 0.05) < 1e-9
    assert desc.rows == b.pose_rows.data_ptr() and desc.counts == b.pose_counts.data_ptr() and desc.frame_info == b.frame_info.data_ptr()
    assert tuple(b.pose_rows.shape) == (B, 100, 36) and tuple(b.pose_counts.shape) == (B,) and b.pose_counts.dtype == torch.int32
    assert b.tagged == a.tagged and b.flops == a.flops and not hasattr(a, 'pose_rows')
    assert a.check_stream_ordering() == [] and b.check_stream_ordering() == []
    # the race check sees the new op: what it reads is what the decode and the polling wrote
    reads, writes = b.access[-1]
    assert set(R.Plan.spans([b.keypoints, b.residuals, b.scores, b.boxes])) <= set(reads) and set(R.Plan.spans([b.pose_rows, b.pose_counts])) == set(writes)


def test_pose_calls_need_a_pose_model(cpu_models):
    plain, posed = cpu_models['f32']
    with pytest.raises(hip.GppError):
        plain.predict_poses_on_batch([np.zeros((1, 96, 160, 3), np.float32), np.zeros((1, 4, 3), np.float32), np.ones((1, 4, 4), np.float32)], 1.0, (96, 160, 3))
    with pytest.raises(hip.GppError):
        plain.predict_poses_on_frames(np.zeros((1, 96, 160, 3), np.uint8), np.zeros((1, 4, 3), np.float32), np.ones((1, 4, 4), np.float32))
    assert posed.pose and not plain.pose
