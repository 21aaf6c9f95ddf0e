""" Ragged batches without a GPU: the height classes of utils/image.py, the per-image tap tables, ragged plans built on the CPU
device (as tests/test_plan_cpu.py builds plans), what the new entry points refuse on the host before any launch, and the grouping of
bin/run_network.py. """
import ctypes
import os

import numpy as np
import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import image as I

KITTI = {(375, 1242): (402, 1333), (370, 1224): (403, 1333), (374, 1238): (403, 1333), (376, 1241): (404, 1333)}


def test_height_class_of_the_four_kitti_sizes():
    for raw, resized in KITTI.items():
        assert I.resized_shape(raw)[:2] == resized
        assert I.height_class(raw) == I.height_class(raw + (3,)) == (101, 1333)
    assert I.split_by_height_class(list(KITTI)) == [((101, 1333), [0, 1, 2, 3])]
    assert I.split_by_height_class([(375, 1242), (200, 1242), (376, 1241)]) == [((101, 1333), [0, 2]), (I.height_class((200, 1242)), [1])]


@pytest.mark.parametrize('Hp', [1, 2, 24, 101, 200])
def test_the_heights_of_a_class(Hp):
    lo, hi = I.class_height_range(Hp)
    assert (lo, hi) == (4 * Hp - 3, 4 * Hp)
    assert [I.class_of_resized(h, 160) for h in range(lo, hi + 1)] == [(Hp, 160)] * 4
    assert I.class_of_resized(hi + 1, 160) == (Hp + 1, 160) and I.class_of_resized(lo - 1, 160) == (Hp - 1, 160)
    for h in range(lo, hi + 1):          # the class is the pool1 shape of the uniform stem (models/builder.py resnet_backbone)
        H1 = (h + 6 - 7) // 2 + 1
        assert (H1 + 1) // 2 == Hp


def test_per_image_taps_are_those_of_each_image_alone():
    shapes = [(374, 1238), (375, 1242), (376, 1241), (370, 1224)]
    cls, heights, scales, (y0, y1, wy, x0, x1, wx) = I.ragged_taps(shapes)
    assert cls == (101, 1333) and heights.tolist() == [403, 402, 404, 403] and heights.dtype == np.int32
    assert y0.shape == y1.shape == wy.shape == (4, 404) and x0.shape == x1.shape == wx.shape == (4, 1333)
    assert y0.dtype == x1.dtype == np.int32 and wy.dtype == wx.dtype == np.float32
    for b, shape in enumerate(shapes):
        scale = I.compute_resize_scale(shape)
        assert scales[b] == scale
        H = heights[b]
        for got, want in zip((y0[b, :H], y1[b, :H], wy[b, :H]), I._axis_taps(H, shape[0], scale)):
            assert np.array_equal(got, want) and not np.any(got[H:])
        for got, want in zip((x0[b], x1[b], wx[b]), I._axis_taps(1333, shape[1], scale)):
            assert np.array_equal(got, want)
    with pytest.raises(ValueError, match=r'\(101, 1333\).*\(51, 1333\)|\(51, 1333\).*\(101, 1333\)'):
        I.ragged_taps([(375, 1242), (188, 1242)])


@pytest.fixture(scope='module')
def cpu_model():
    weights, built = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def model_for(bb, dt, **kw):
            key = (bb, dt, tuple(sorted(kw.items())))
            if key not in built:
                if bb not in weights:
                    weights[bb] = W.synthetic_weights(bb, 1234)
                built[key] = models.load_model(weights[bb], backbone_name=bb, dtype=dt, **kw)
            return built[key]
        yield model_for


def op_shape(plan, pos):
    io = plan.op_io[pos]
    return None if io is None else tuple(tuple((f.B, f.H, f.W, f.C, f.pitch) for f in part or ()) for part in io)


@pytest.mark.parametrize('fuse', ['1', '0'])
@pytest.mark.parametrize('dtype', ['f16x3', 'bf16x3', 'f32', 'bf16', 'f16'])
def test_a_ragged_plan_is_the_uniform_plan_behind_pool1(dtype, fuse, cpu_model, monkeypatch):
    monkeypatch.setenv('GPP_FUSE_STEM_POOL', fuse)
    model = cpu_model('resnet50', dtype)
    model._plans.clear()
    uniform = model.plan_for(4, 96, 160, 100, True)
    ragged = model.plan_for(4, 96, 160, 100, True, ragged=True)
    keys = list(model._plans)
    model._plans.clear()
    assert keys == [(4, 96, 160, 100, True), (4, ('class', 24), 160, 100, True)]
    assert ragged.ragged and not uniform.ragged and ragged.heights.dtype == torch.int32 and ragged.heights.tolist() == [96] * 4
    assert ragged.check_stream_ordering() == []
    fused = any(kind == R.OP_STEM_POOL for kind, *_ in uniform.ops)
    assert fused == (fuse == '1' and dtype != 'f32')
    n = 1 if fused else 2
    want = [R.OP_STEM_POOL_RAGGED] if fused else [R.OP_STEM_RAGGED, R.OP_MAXPOOL_RAGGED]
    assert [op[0] for op in ragged.ops[:n]] == want and [op[3] for op in ragged.ops[:n]] == [op[3] for op in uniform.ops[:n]]
    for op in ragged.ops[:n]:
        d = op[2]
        assert d.heights == ragged.heights.data_ptr() and d.Hp == 24
        assert (d.stem.H if hasattr(d, 'stem') else d.pool.H) == (96 if hasattr(d, 'stem') else 48)
    assert len(ragged.ops) == len(uniform.ops)
    for pos in range(n, len(uniform.ops)):
        a, b = uniform.ops[pos], ragged.ops[pos]
        assert (a[0], a[1], a[3], a[4]) == (b[0], b[1], b[3], b[4]) and uniform.lanes[pos] == ragged.lanes[pos], a[3]
        assert op_shape(uniform, pos) == op_shape(ragged, pos), a[3]
    assert not any(op[0] in (R.OP_STEM, R.OP_STEM_POOL, R.OP_MAXPOOL) for op in ragged.ops)


def test_latency_and_pose_models_build_ragged_plans(cpu_model):
    for kw in ({'plan': 'latency'}, {'pose': True}):
        model = cpu_model('resnet101', 'f16x3', **kw)
        plan = model.plan_for(2, 404, 1333, 100, True, ragged=True)
        model._plans.clear()
        assert plan.check_stream_ordering() == [] and plan.ops[0][0] == R.OP_STEM_POOL_RAGGED


def test_heights_outside_the_class_and_lists_over_two_classes_are_refused(cpu_model):
    model = cpu_model('resnet50', 'f16x3')
    plan = model.plan_for(2, 96, 160, 100, True, ragged=True)
    model.put_heights(plan, [93, 96])
    assert plan.heights.tolist() == [93, 96] and plan.heights_host == [93, 96]
    for bad in ([92, 96], [96, 97], [96], [0, 96]):
        with pytest.raises(ValueError):
            model.put_heights(plan, bad)
    assert plan.heights.tolist() == [93, 96]
    P_inv, planes = np.zeros((2, 4, 3), np.float32), np.zeros((100, 4), np.float32)
    a, b, c = (np.zeros((h, 160, 3), np.float32) for h in (94, 96, 97))
    staged = model.stage_inputs([[a, b], P_inv, planes])
    assert staged.ragged and staged.heights.tolist() == [94, 96] and tuple(staged.images.shape) == (2, 96, 160, 3)
    with pytest.raises(ValueError, match=r'\(24, 160\) and \(25, 160\)'):
        model.stage_inputs([[a, c], P_inv, planes])
    with pytest.raises(ValueError, match=r'\(24, 160\) and \(24, 164\)'):
        model.stage_inputs([[a, np.zeros((94, 164, 3), np.float32)], P_inv, planes])
    model._plans.clear()


@pytest.mark.parametrize('backbone', ['mobilenet224_1.0', 'densenet121'])
def test_backbones_without_a_ragged_form_say_so(backbone, cpu_model):
    model = cpu_model(backbone, 'f16x3')
    assert not model.supports_ragged
    images = [np.zeros((h, 160, 3), np.float32) for h in (94, 96)]
    with pytest.raises(ValueError, match='no ragged form'):
        model.stage_inputs([images, np.zeros((2, 4, 3), np.float32), np.zeros((100, 4), np.float32)])
    assert not model._plans


def test_audit_models_pipelines_and_sharded_models_refuse_a_list(cpu_model):
    from keras_retinanet_3D.utils import distributed, pipeline
    inputs = [[np.zeros((h, 160, 3), np.float32) for h in (94, 96)], np.zeros((2, 4, 3), np.float32), np.zeros((100, 4), np.float32)]
    audit = cpu_model('resnet50', 'f16x3', range_audit=True)
    with pytest.raises(ValueError, match='no ragged form'):
        audit.stage_inputs(inputs)
    model = cpu_model('resnet50', 'f16x3')
    with pytest.raises(ValueError, match='ragged'):
        distributed.ShardedModel(model).predict_on_batch(inputs)
    pipe = pipeline.FramePipeline.__new__(pipeline.FramePipeline)          # (its constructor makes streams: the refusal comes before any use)
    pipe.depth, pipe.slots = 4, None
    with pytest.raises(ValueError, match='ragged'):
        next(pipe.run([([np.zeros((94, 160, 3), np.uint8)], inputs[1], inputs[2])]))


# ---------------------------------------------------------------------------------------------------- the C ABI, on the host
def ragged_calls():
    """ (name, call(heights, rows, Hp) -> rc) of every new entry point, with valid dummy pointers: each must return before any launch """
    lib = hip.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    return [
        ('gpp_stem_conv7x7_bn_relu_ragged', lambda h, rows, Hp: lib.gpp_stem_conv7x7_bn_relu_ragged(p, p, p, p, hip.GPP_F32, 2, rows, 160, Hp, h, None)),
        ('gpp_stem_conv7x7_bn_relu_mfma_ragged', lambda h, rows, Hp: lib.gpp_stem_conv7x7_bn_relu_mfma_ragged(p, p, p, p, hip.GPP_F16, 2, rows, 160, Hp, h, None)),
        ('gpp_stem_conv7x7_bn_relu_x3_rc_ragged', lambda h, rows, Hp: lib.gpp_stem_conv7x7_bn_relu_x3_rc_ragged(p, p, p, p, 2, rows, 160, Hp, h, None, None)),
        ('gpp_stem_pool_fused_mfma_ragged', lambda h, rows, Hp: lib.gpp_stem_pool_fused_mfma_ragged(p, p, p, p, hip.GPP_BF16, 2, rows, 160, Hp, h, None)),
        ('gpp_stem_pool_fused_x3_ragged', lambda h, rows, Hp: lib.gpp_stem_pool_fused_x3_ragged(p, p, p, p, 2, rows, 160, Hp, h, None, None)),
        ('gpp_maxpool3x3s2_same_ragged', lambda h, rows, Hp: lib.gpp_maxpool3x3s2_same_ragged(p, p, hip.GPP_F32, 2, rows // 2, 80, 64, Hp, h, None)),
        ('gpp_preprocess_u8_bgr_ragged', lambda h, rows, Hp: lib.gpp_preprocess_u8_bgr_ragged(p, p, p, h, p, p, p, p, p, p, 2, 90, 150, Hp, rows, 160,
                                                                                            103.939, 116.779, 123.68, None)),
    ], p


def test_every_ragged_entry_point_checks_its_arguments_before_any_launch():
    calls, p = ragged_calls()
    odd = ctypes.c_void_p(p.value + 2)
    for name, call in calls:
        assert call(None, 96, 24) == -1, name                     # no table
        assert call(p, 100, 24) == -1, name                       # canvas rows that are not the class's 4 Hp (the pool: 2 Hp)
        assert call(p, 96, 25) == -1, name
        assert call(p, 0, 0) == -1, name
        assert call(odd, 96, 24) == -3, name                      # a table that is not 4-byte aligned
    lib = hip.lib()
    assert lib.gpp_stem_pool_fused_x3_ragged(None, p, p, p, 2, 96, 160, 24, p, None, None) == -1
    assert lib.gpp_preprocess_u8_bgr_ragged(p, p, None, p, p, p, p, p, p, p, 2, 90, 150, 24, 96, 160, 0.0, 0.0, 0.0, None) == -1


def test_the_plan_runner_knows_the_ragged_kinds():
    """ gpp_plan_run forwards the new kinds to the entry points above: a descriptor they refuse comes back as their error, not as an unknown kind """
    d = R.RaggedStemDesc(R.StemDesc(1, 1, 1, 16, hip.GPP_F16, 2, 100, 160, None), 4, 24, 0)
    pd = R.RaggedPoolDesc(R.PoolDesc(16, 16, hip.GPP_F16, 2, 50, 80, 64, 0), 4, 24, 0)
    for kind, desc in ((R.OP_STEM_RAGGED, d), (R.OP_STEM_POOL_RAGGED, d), (R.OP_MAXPOOL_RAGGED, pd)):
        op = R.PlanOp(kind, 0, ctypes.addressof(desc))
        assert hip.lib().gpp_plan_run(ctypes.byref(op), 1, None, None, 0) == -1
    assert (R.OP_STEM_RAGGED, R.OP_STEM_POOL_RAGGED, R.OP_MAXPOOL_RAGGED) == (37, 38, 39)


# ---------------------------------------------------------------------------------------------------- bin/run_network.py
def test_run_network_groups_the_four_kitti_sizes_into_one_call():
    from keras_retinanet_3D.bin import run_network

    class Ragged(object):
        supports_ragged = True

    class Uniform(object):
        pass

    items = [{'raw_image': np.zeros(s + (3,), np.uint8)} for s in KITTI]
    groups = run_network.group_items(Ragged(), items)
    assert len(groups) == 1 and groups[0][1] is True and [id(it) for it in groups[0][0]] == [id(it) for it in items]
    assert [(len(g), r) for g, r in run_network.group_items(Uniform(), items)] == [(1, False)] * 4
    same = [items[0], dict(items[0])]
    assert [(len(g), r) for g, r in run_network.group_items(Ragged(), same)] == [(2, False)]          # one shape: an array, as ever
    far = items[:2] + [{'raw_image': np.zeros((200, 1242, 3), np.uint8)}]
    assert [(len(g), r) for g, r in run_network.group_items(Ragged(), far)] == [(2, True), (1, False)]
