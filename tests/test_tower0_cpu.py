""" Layer 0 of the regression tower on the 9 x 9 candidate set in plans built without a GPU: head_forms names the form
at GPP_SPARSE_TOWER_DEPTH >= 4 only, the flagship plan keeps its ops, FLOPs and lanes, every kind of plan that keeps the fused launch is the
same plan at depth 3 and 4, and Plan.check_stream_ordering sees what pyramid_classification's op now reads and writes. """
import os

import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import plan as P
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W

TOWER0, CLS, LAYER1 = 'pyramid_towers_0', 'pyramid_classification', 'pyramid_regression_1'


@pytest.fixture(scope='module')
def build():
    weights = W.synthetic_weights('resnet50', 1234)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def plan_for(B, H, Wd, depth, env=(), **kw):
            env = dict(env, GPP_SPARSE_TOWER_DEPTH=str(depth))
            for k, v in env.items():
                mp.setenv(k, v)
            try:
                return models.load_model(weights, backbone_name='resnet50', dtype='f16x3', **kw).plan_for(B, H, Wd, 100, True)
            finally:
                for k in env:
                    mp.delenv(k)
        yield plan_for


@pytest.fixture(scope='module')
def flagship(build):
    return {depth: build(8, 402, 1333, depth) for depth in (3, 4)}


def same_ops(a, b):
    assert len(a.ops) == len(b.ops) and a.flops == b.flops and a.lanes == b.lanes and a.tagged == b.tagged
    for x, y in zip(a.ops, b.ops):
        assert (x[0], x[1], x[3], x[4]) == (y[0], y[1], y[3], y[4])          # kind, tag, name, flops


def towers_0(plan):
    return [d for kind, _, d, name, _ in plan.ops if name == TOWER0]


LEVELS = [(51, 167), (26, 84), (13, 42), (7, 21), (4, 11)]          # 402 x 1333
SHAPES = dict({n: (3, 3, 512, 512) for n in ('pyramid_regression_1', 'pyramid_regression_2', 'pyramid_regression_3')},
              pyramid_classification=(3, 3, 256, 96), pyramid_regression_ops=(3, 3, 512, 144), pyramid_regression_dim=(3, 3, 128, 36),
              pyramid_towers_0=(3, 3, 512, 896))


def options(**fields):
    base = dict(sparse_heads=0.5, sparse_tower=0.75, sparse_tower_rounds=1.0, sparse_deep=0.75, sparse_deep_rounds=1.0, sparse_depth=4,
                decode_overlap=True, x3_level=2, cls_lane=0, head_lanes=False)
    return P.PlanOptions(**{f: dict(base, **fields).get(f) for f in P.PlanOptions._fields})


def forms_of(opts=None, dtype='f16x3', plan_mode='throughput', osf=False, audit=False, layers=SHAPES, deep_lists=True, levels=LEVELS, B=8, **kw):
    return P.head_forms(opts or options(), dtype, plan_mode, osf, audit, layers, deep_lists, levels, B, **kw)


def test_head_forms_names_layer_0_at_depth_4_only_and_on_each_condition():
    pair = {'pyramid_classification': 'lists_after', 'pyramid_regression_ops': 'pair', 'pyramid_regression_dim': 'pair'}
    assert forms_of() == P.HeadForms(True, pair, True, 2, True)
    three = forms_of(options(sparse_depth=3))
    assert three == P.HeadForms(True, pair, True, 2, False) == P.HeadForms(True, pair, True, 2)         # the new field has a default
    assert forms_of(options(sparse_depth=2)).tower0 is False and forms_of(options(sparse_depth=1)).tower0 is False
    assert forms_of(options(sparse_depth=9)).tower0 is True
    # every condition of the deep form is one of this form: whatever refuses layers 1 and 2 refuses layer 0
    for refused in (forms_of(options(cls_lane=2)), forms_of(options(head_lanes=True)), forms_of(osf=True), forms_of(audit=True),
                    forms_of(deep_lists=False), forms_of(options(sparse_tower=0.0)), forms_of(options(sparse_heads=0.0, sparse_tower=0.0)),
                    forms_of(dtype='f32'), forms_of(B=1)):
        assert refused.tower0 is False and refused.deep_layers == 0
    # ... and its own: the entry point, the throughput plan, a map that has the slice in front of other columns, the rounds
    assert forms_of(deferred=False) == three
    assert forms_of(plan_mode='latency').tower0 is False
    assert forms_of(layers={k: v for k, v in SHAPES.items() if k != TOWER0}) == three
    assert forms_of(layers=dict(SHAPES, pyramid_towers_0=(3, 3, 512, 512))) == three
    rows = sum((8 * h * w + 255) // 256 for h, w in LEVELS)              # rows of 256 x 256 workgroups, two columns of them
    assert forms_of(options(sparse_deep_rounds=(2 * rows - 1) / 256.0)).tower0 is True
    assert forms_of(options(sparse_deep_rounds=2 * rows / 256.0)).deep_layers == 0
    # callers that build the tuples positionally, as before this form existed, still work
    assert P.HeadForms(False, {}, False, 0).tower0 is False


def test_the_flagship_plan_keeps_its_ops_and_splits_the_first_layer(flagship):
    three, four = flagship[3], flagship[4]
    same_ops(four, three)
    assert three.check_stream_ordering() == [] and four.check_stream_ordering() == []
    sp = four.sparse
    assert three.sparse.tower0 is None and three.sparse.tower0_tensors() == [] and towers_0(three)[0].C_out == 896
    (rest,), first = towers_0(four), sp.tower0
    assert (rest.C_out, first.C_out, rest.C_in, first.C_in) == (384, 512, 512, 512) and rest.out_pitch == first.out_pitch == 896
    itemsize, k = 4, 9 * 512
    assert rest.weight - first.weight == 512 * k * itemsize and rest.bias - first.bias == 512 * 4 and rest.out_scale - first.out_scale == 512 * 4
    assert [g.out_off - h.out_off for g, h in zip(rest.groups[:5], first.groups[:5])] == [512] * 5
    # the slice is a layer of both forms on lists of its own, not a member of the deep_* lists, and no op of the plan
    assert first.deep_rows == sp.tower0_rows.data_ptr() and first.deep_counts == sp.tower0_counts.data_ptr() and first.deep_flag == sp.tower0_flag.data_ptr()
    assert sp.deep_layers == 2 and len(sp.deep) == 2 and len(sp.deep_flags) == 2 and len(sp.deep_stats) == 4 and first not in [op[2] for op in four.ops]
    assert int(sp.tower0_flag.item()) == 1                                     # dense until a run's lists say otherwise
    names = [op[3] for op in four.ops]
    cls = four.ops[names.index(CLS)][2]
    assert sp.tower0_handle > 0 and cls.conv_after == sp.tower0_handle and cls.lists_after == sp.deep_handle
    assert hip.lib().gpp_conv2d_deferred_run(sp.tower0_handle, 1, None) == 0
    assert three.ops[names.index(CLS)][2].conv_after == 0
    # the layer's shape is layer 1's: the same FLOPs, and the op keeps the fused layer's count
    layer1 = four.ops[names.index(LAYER1)]
    assert four.ops[names.index(TOWER0)][4] == layer1[4] * 896 / 512


@pytest.mark.parametrize('shape, env, kw', [
    ((8, 402, 1333), {}, {'range_audit': True}),
    ((8, 402, 1333), {}, {'plan': 'latency'}),
    ((2, 402, 1333), {}, {}),                                           # cls_lane: the logits are written on a side lane
    ((8, 402, 1333), {'GPP_HEAD_LANES': '1'}, {}),
    ((8, 402, 1333), {}, {'orientation_specific_filter': True}),
    ((4, 224, 352), {}, {}),                                            # too few rounds
    ((8, 402, 1333), {'GPP_SPARSE_TOWER_DEEP_MAX_SHARE': '0.5', 'GPP_SPARSE_TOWER': '0'}, {}),
])
def test_plans_that_keep_the_fused_launch_are_the_same_plan_at_depth_3_and_4(build, shape, env, kw):
    three, four = build(*shape, 3, env=env, **kw), build(*shape, 4, env=env, **kw)
    same_ops(four, three)
    assert [op[3] for op in four.ops] == [op[3] for op in three.ops]
    for plan in (three, four):
        assert plan.check_stream_ordering() == []
        assert [d.C_out for d in towers_0(plan)] == [896] and (plan.sparse is None or plan.sparse.tower0 is None)
        assert all(not op[2].conv_after for op in plan.ops if op[0] == R.OP_CONV)


def test_the_ordering_check_needs_what_pyramid_classification_declares(flagship):
    """ pyramid_classification moved to a side lane nobody joins in front of layer 1, and layer 1 reduced to a reader of its input map alone:
    the race on the regression slice is found in the plan that declares the slice under pyramid_classification, not in one that does not """
    def races(plan, strip):
        names = [op[3] for op in plan.ops]
        cls, l1 = names.index(CLS), names.index(LAYER1)
        saved = plan.lanes[cls], plan.access[cls], plan.access[l1]
        src = plan.io[LAYER1][0]
        plan.lanes[cls] |= 3 << 8
        plan.access[l1] = (P.Plan.spans(src), plan.access[l1][1])                 # without the lists, which pyramid_classification writes too
        if strip:
            known = set(P.Plan.spans(src) + P.Plan.spans(plan.sparse.tower0_tensors()))
            plan.access[cls] = (plan.access[cls][0], [iv for iv in plan.access[cls][1] if iv not in known])
        bad = plan.check_stream_ordering()
        plan.lanes[cls], plan.access[cls], plan.access[l1] = saved
        return (CLS, LAYER1) in bad
    three, four = flagship[3], flagship[4]
    assert races(four, strip=False) and not races(four, strip=True) and not races(three, strip=False)
    assert four.check_stream_ordering() == []
    # the declaration itself: the P maps among the reads, the slice and layer 0's lists among the writes
    names = [op[3] for op in four.ops]
    reads, writes = four.access[names.index(CLS)]
    assert set(P.Plan.spans(four.io[TOWER0][0])) <= set(reads)
    assert set(P.Plan.spans(four.io[LAYER1][0]) + P.Plan.spans(four.sparse.tower0_tensors())) <= set(writes)
    reads3, writes3 = three.access[names.index(CLS)]
    assert not set(P.Plan.spans(three.io[TOWER0][0])) & set(reads3) and not set(P.Plan.spans(three.io[LAYER1][0])) & set(writes3)


def test_reading_a_head_tensor_completes_the_slice_in_front_of_layer_1(flagship, monkeypatch):
    """ Plan.complete_heads issues the launches it always did; at depth 4 the first of them, layer 1's dense launch, names layer 0's regression
    slice in front of itself (gpp_conv_desc.conv_before): the library runs its copy dense, into the same scratch counter """
    calls = []
    monkeypatch.setattr(hip.lib(), 'gpp_conv2d_igemm',
                        lambda desc, stream: calls.append((desc._obj.C_out, desc._obj.conv_before, desc._obj.conv_after, desc._obj.deep_rows,
                                                           desc._obj.range_counter)) or 0, raising=False)
    monkeypatch.setattr(hip, 'stream_ptr', lambda: None)
    for depth, plan in flagship.items():
        calls.clear()
        plan.heads_stale = True
        plan.regression
        plan.heads_stale = False
        sp = plan.sparse
        assert [c[0] for c in calls] == [512, 512, 512, 144, 36] and all(c[2] == 0 and c[3] is None for c in calls)
        assert [c[1] for c in calls] == [sp.tower0_handle if depth == 4 else 0, 0, 0, 0, 0] and (sp.tower0_handle > 0) == (depth == 4)
        assert calls[0][4] == sp.range_scratch.data_ptr() != plan.range_slot.data_ptr()
