""" Shared helpers for the test-suite (oracle access, golden loading). """
import ctypes
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def polling_golden_names():
    return sorted(os.path.basename(p)[len('polling_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'polling_*.npz')))


def load_polling_golden(name):
    from keras_retinanet_3D.utils import synthetic
    g = dict(np.load(os.path.join(GOLDEN, 'polling_{}.npz'.format(name))))
    g['planes'] = synthetic.load_plane_database(str(g['db'])).astype(np.float32)
    return g


def resize_golden_names():
    return sorted(os.path.basename(p)[len('resize_'):-len('.npz')] for p in glob.glob(os.path.join(GOLDEN, 'resize_*.npz')))


def load_resize_golden(name):
    """ tests/golden/resize_<name>.npz (oracle/gen_resize_goldens.py): the reference's resize_image(preprocess_image(frame), min_side,
    max_side) with oracle/image_np as its cv2.resize; the scalars as Python floats """
    g = dict(np.load(os.path.join(GOLDEN, 'resize_{}.npz'.format(name))))
    for k in ('min_side', 'max_side', 'fx', 'fy', 'scale'):
        g[k] = float(g[k])
    return g


def c_oracle_poll(lib, boxes, dims, orient, P_inv, planes, thr=0.7):
    """ oracle/polling.c through ctypes; planes (N,4) shared or (B,N,4). """
    boxes = np.ascontiguousarray(boxes, np.float32)
    dims = np.ascontiguousarray(dims, np.float32)
    orient = np.ascontiguousarray(orient, np.int32)
    P_inv = np.ascontiguousarray(P_inv, np.float32)
    planes = np.ascontiguousarray(planes, np.float32)
    B, D = boxes.shape[:2]
    batched = int(planes.ndim == 3)
    N = planes.shape[-2]
    kp = np.empty((B, D, 4, 3), np.float32)
    kpl = np.empty((B, D, 1, 4), np.float32)
    res = np.empty((B, D), np.float32)
    idx = np.empty((B, D), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.gpp_oracle_poll_f32.restype = ctypes.c_int
    rc = lib.gpp_oracle_poll_f32(p(boxes), p(dims), p(orient), p(P_inv), p(planes), B, D, N, batched,
                                 ctypes.c_float(thr), p(kp), p(kpl), p(res), p(idx))
    assert rc == 0
    return kp, kpl, res, idx


def bits_equal(a, b):
    """ bitwise equality of float arrays (NaN == NaN, +0 != -0 is tolerated as equal). """
    a = np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# every switch of the plan builder (GPP_* variables read by models/plan.plan_options when a plan is built): the GPU test runs each against the one-stream plan
# (tests/test_network_gpu.py), the CPU test (tests/test_plan_cpu.py) checks the stream ordering and the descriptors of each at several batches
PLAN_OPTIONS = [{}, {'GPP_HALF_LANES': '1,2'}, {'GPP_HALF_LANES': '1'}, {'GPP_HALF_LANES': '2'}, {'GPP_HALF_LANES': '0,1,2,3'}, {'GPP_HALF_LANES': '0,2'},
                {'GPP_HALF_LANES': ''}, {'GPP_BR1_LANE': '0'}, {'GPP_FPN_LANES': '0'}, {'GPP_P4_LANE': '0'}, {'GPP_HEAD_LANES': '1'},
                {'GPP_DECODE_OVERLAP': '0'}, {'GPP_STAGE_CHUNKS': '4,8,8,8'}, {'GPP_STAGE_CHUNKS': '2,4,8,8', 'GPP_HALF_LANES': '2,3'},
                {'GPP_HALF_LANES': '3', 'GPP_FPN_LANES': '0', 'GPP_BR1_LANE': '0'}, {'GPP_CLS_LANE': '1'}, {'GPP_CLS_LANE': '1', 'GPP_HALF_LANES': ''},
                {'GPP_HALF_LANES': '1,2,3'}, {'GPP_FUSE_BLOCK': ''}, {'GPP_FUSE_BLOCK': '64,128', 'GPP_FUSE_BLOCK_PROJ': '1'}]      # (round 6: the old default; no fused blocks; projection blocks fused too)


def plan_matrix():
    """ the plan configurations tests/test_plan_cpu.py checks and tools/plan_fingerprint.py hashes, each as
    (backbone, dtype, model keyword arguments, environment, B, H, W) """
    small = (200, 333)
    cfgs = [('resnet50', dt, {}, env, b) + small for env in PLAN_OPTIONS for dt in ('f16x3', 'bf16x3', 'f32', 'bf16', 'f16') for b in (1, 2, 3, 8)]
    cfgs += [(bb, 'f16x3', {}, {}, 4) + small for bb in ('resnet101', 'resnet152')]
    cfgs += [('densenet121', dt, {}, {}, b) + small for dt in ('f32', 'f16x3', 'bf16x3') for b in (1, 2)]
    cfgs += [('resnet50', 'f16x3', kw, {}, b) + small for kw in ({'plan': 'latency'}, {'orientation_specific_filter': True}, {'nms': False})
             for b in (1, 4)]
    cfgs += [('resnet50', dt, {}, env, 4) + small for dt in ('f16x3', 'bf16x3', 'bf16')
             for env in ({'GPP_X3_SPLIT': '0'}, {'GPP_X3_SPLIT': '1'}, {'GPP_FUSE_TAIL': ''}, {'GPP_FUSE_STEM_POOL': '0'})]
    cfgs += [('resnet50', 'f16x3', {}, {}, 8, 402, 1333)]
    # 224 x 352 with both round thresholds at 0: the smallest shape at which the regression tower takes its sparse and deep forms (at
    # 200 x 333 pyramid_regression_ops is split-K and stays dense), every type, every switch those forms depend on, the other backbones
    tower, Z = (224, 352), {'GPP_SPARSE_TOWER_MIN_ROUNDS': '0', 'GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS': '0'}
    cfgs += [('resnet50', 'f16x3', {}, Z, 1) + tower] + [('resnet50', dt, {}, Z, 4) + tower for dt in ('f16x3', 'bf16x3', 'bf16', 'f32')]
    cfgs += [('resnet50', 'f16x3', {}, dict(Z, **env), 4) + tower
             for env in ({'GPP_SPARSE_TOWER_DEPTH': '1'}, {'GPP_SPARSE_TOWER_DEPTH': '2'}, {'GPP_SPARSE_TOWER': '0'}, {'GPP_SPARSE_HEADS': '0'},
                         {'GPP_CLS_LANE': '1'}, {'GPP_HEAD_LANES': '1'}, {'GPP_X3_SPLIT': '0'}, {'GPP_DECODE_OVERLAP': '0'})]
    cfgs += [('resnet50', 'f16x3', kw, Z, 4) + tower for kw in ({'plan': 'latency'}, {'orientation_specific_filter': True}, {'pose': True})]
    cfgs += [('densenet121', 'f16x3', {}, Z, 2) + tower, ('mobilenet224_1.0', 'f16x3', {}, Z, 4) + tower]
    # ... and at the default thresholds: the same shape, MobileNet, the pose stage with and without the cuboid NMS, audit plans, the
    # latency plan at full size, and ragged plans ('ragged' is no model argument: both consumers of the matrix pop it for plan_for)
    cfgs += [('resnet50', 'f16x3', {}, {}, 4) + tower, ('mobilenet224_1.0', 'f16x3', {}, {}, 2) + small, ('mobilenet224_1.0', 'f32', {}, {}, 1) + small]
    cfgs += [('resnet50', 'f16x3', kw, {}, 2) + small for kw in ({'pose': True}, {'pose': True, 'cuboid_nms': ('bev', 0.5)}, {'range_audit': True})]
    cfgs += [('densenet121', 'f16x3', {'range_audit': True}, {}, 1) + small, ('resnet50', 'f16x3', {'plan': 'latency'}, Z, 8, 402, 1333)]
    cfgs += [('resnet50', dt, {'ragged': True}, env, b, 192, 333)
             for dt, env, b in (('f16x3', {}, 3), ('bf16', {}, 3), ('f16x3', {'GPP_FUSE_STEM_POOL': '0'}, 2))]
    return cfgs


def plan_label(cfg):
    bb, dt, kw, env, B, H, Wd = cfg
    return ' '.join([bb, dt, 'B={}'.format(B), '{}x{}'.format(H, Wd)] + ['{}={}'.format(*kv) for kv in sorted(kw.items())] +
                    ['{}={}'.format(*kv) for kv in sorted(env.items())])
