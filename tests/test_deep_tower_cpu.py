""" Deep sparse regression tower in plans built without a GPU: layers 1 and 2 of the regression tower stay ONE op each
with the tower's tag and the algorithmic FLOPs and read the lists that pyramid_classification's op writes on the same stream (no join to
find); the ops of a plan do not change with the depth; and only plans that meet every condition of the rule take the form. """
import os

import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W

LAYER1, LAYER2, LAYER3, CLS = 'pyramid_regression_1', 'pyramid_regression_2', 'pyramid_regression_3', 'pyramid_classification'


@pytest.fixture(scope='module')
def build():
    weights = W.synthetic_weights('resnet50', 1234)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def plan_for(B, H, Wd, env=(), **kw):
            for k, v in dict(env).items():
                mp.setenv(k, v)
            try:
                return models.load_model(weights, backbone_name='resnet50', dtype='f16x3', **kw).plan_for(B, H, Wd, 100, True)
            finally:
                for k in dict(env):
                    mp.delenv(k)
        yield plan_for


def deep_ops(plan):
    return [i for i, (kind, _, desc, _, _) in enumerate(plan.ops) if kind == R.OP_CONV and desc.deep_rows]


def list_ops(plan):
    return [i for i, (kind, _, desc, _, _) in enumerate(plan.ops) if kind == R.OP_CONV and desc.lists_after]


def carries_nothing(plan):
    sp = plan.sparse
    return not deep_ops(plan) and not list_ops(plan) and (sp is None or (sp.deep == [] and sp.deep_layers == 0 and sp.deep_tensors() == []))


@pytest.fixture(scope='module')
def flagship(build):
    return {depth: build(8, 402, 1333, env={'GPP_SPARSE_TOWER_DEPTH': str(depth)}) for depth in (1, 2, 3)}


def test_the_flagship_plan_carries_the_deep_fields_and_orders_their_reads(build, flagship):
    plan = build(8, 402, 1333)                  # the default depth
    sp = plan.sparse
    names = [op[3] for op in plan.ops]
    assert sp is not None and sp.deep_layers == 2 and plan.check_stream_ordering() == []
    assert [names[i] for i in deep_ops(plan)] == [LAYER1, LAYER2] and [names[i] for i in list_ops(plan)] == [CLS]
    d1, d2 = plan.ops[names.index(LAYER1)][2], plan.ops[names.index(LAYER2)][2]
    assert sp.deep == [d1, d2]
    for desc, which in ((d2, 0), (d1, 1)):      # layer 2 on the radius-2 lists, layer 1 on the radius-3 lists
        assert desc.deep_rows == sp.deep_rows[which].data_ptr() and desc.deep_counts == sp.deep_counts[which].data_ptr()
        assert desc.deep_flag == sp.deep_flags[which].data_ptr()
        assert not desc.tower_rows and not desc.gather_rows and not desc.guard and not desc.lists_after
    assert [int(f.item()) for f in sp.deep_flags] == [1, 1]             # dense until a run's lists say otherwise
    # the only op with tower_rows is still the last layer; the tag-1 list is what it was
    assert [names[i] for i, op in enumerate(plan.ops) if op[0] == R.OP_CONV and op[2].tower_rows] == [LAYER3] and sp.tower == [plan.ops[names.index(LAYER3)][2]]
    assert [n for _, t, _, n, _ in plan.ops if t == 1] == [LAYER1, LAYER2, LAYER3]
    # the writer: pyramid_classification on the caller's stream, in front of the candidate pass's fork and of both readers, without a join
    cls = names.index(CLS)
    assert (plan.lanes[cls] >> 8) & 0xff == 0 and cls < names.index('filtered_detections/candidates') < names.index(LAYER1) < names.index(LAYER2)
    assert all((plan.lanes[names.index(n)] >> 8) & 0xff == 0 and not plan.lanes[names.index(n)] & R.OP_JOIN for n in (LAYER1, LAYER2))
    assert sp.deep_handle > 0 and plan.ops[cls][2].lists_after == sp.deep_handle
    assert hip.lib().gpp_detect_deep_lists_run(sp.deep_handle, 1, None) == 0
    # check_stream_ordering sees the new buffers: a reader moved to a side lane nobody forked behind the writer... is found
    pos = names.index(LAYER2)
    saved = plan.lanes[pos]
    plan.lanes[pos] = (2 << 8)
    plan.lanes[cls], saved_cls = plan.lanes[cls] | (3 << 8), plan.lanes[cls]
    bad = plan.check_stream_ordering()
    plan.lanes[pos], plan.lanes[cls] = saved, saved_cls
    assert (CLS, LAYER2) in bad and plan.check_stream_ordering() == []
    same = flagship[3]
    assert [op[3] for op in same.ops] == names and same.sparse.deep_layers == 2


def test_the_depth_changes_neither_ops_nor_flops_nor_lanes(flagship):
    one, two, three = flagship[1], flagship[2], flagship[3]
    assert carries_nothing(one) and one.sparse.tower_rows is not None
    names2 = [op[3] for op in two.ops]
    assert [names2[i] for i in deep_ops(two)] == [LAYER2] and two.sparse.deep_layers == 1 and len(two.sparse.deep) == 1
    assert two.sparse.deep[0].deep_rows == two.sparse.deep_rows[0].data_ptr()
    for plan in (two, three):
        assert len(plan.ops) == len(one.ops) and plan.flops == one.flops and plan.lanes == one.lanes
        for a, b in zip(plan.ops, one.ops):
            assert (a[0], a[1], a[3], a[4]) == (b[0], b[1], b[3], b[4])          # kind, tag, name, flops
        assert plan.tagged == one.tagged and plan.check_stream_ordering() == []


@pytest.mark.parametrize('shape, env, kw', [
    ((4, 224, 352), {}, {}),
    ((4, 224, 352), {'GPP_SPARSE_TOWER_MIN_ROUNDS': '0'}, {}),          # the tower's own variable does not open the deep form
    ((2, 96, 160), {}, {}),
    ((2, 96, 160), {'GPP_SPARSE_TOWER_MIN_ROUNDS': '0', 'GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS': '0'}, {}),      # the split regression output reads every row
    ((2, 402, 1333), {}, {}),                                           # cls_lane: the logits are written on a side lane
    ((2, 402, 1333), {'GPP_SPARSE_TOWER_MIN_ROUNDS': '0', 'GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS': '0'}, {}),
    ((8, 402, 1333), {}, {'range_audit': True}),
    ((8, 402, 1333), {}, {'orientation_specific_filter': True}),
    ((8, 402, 1333), {'GPP_SPARSE_TOWER': '0'}, {}),
    ((8, 402, 1333), {'GPP_SPARSE_HEADS': '0'}, {}),
    ((8, 402, 1333), {'GPP_HEAD_LANES': '1'}, {}),
])
def test_plans_that_do_not_take_the_form(build, shape, env, kw):
    plan = build(*shape, env=env, **kw)
    assert carries_nothing(plan) and plan.check_stream_ordering() == []


def test_a_small_plan_takes_the_form_when_both_round_rules_are_lifted(build):
    plan = build(4, 224, 352, env={'GPP_SPARSE_TOWER_MIN_ROUNDS': '0', 'GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS': '0'})
    names = [op[3] for op in plan.ops]
    assert [names[i] for i in deep_ops(plan)] == [LAYER1, LAYER2] and plan.check_stream_ordering() == []


def test_reading_a_head_tensor_runs_the_deep_layers_dense_first(build, monkeypatch):
    plan = build(8, 402, 1333)
    calls = []
    monkeypatch.setattr(hip.lib(), 'gpp_conv2d_igemm',
                        lambda desc, stream: calls.append((desc._obj.C_out, desc._obj.deep_rows, desc._obj.tower_rows, desc._obj.guard,
                                                           desc._obj.range_counter, desc._obj.inp, desc._obj.lists_after)) or 0, raising=False)
    monkeypatch.setattr(hip, 'stream_ptr', lambda: None)
    plan.heads_stale = True
    plan.regression
    assert [c[0] for c in calls] == [512, 512, 512, 144, 36]
    assert all(c[1] is None and c[2] is None and c[3] is None and c[6] == 0 for c in calls)
    scratch = plan.sparse.range_scratch.data_ptr()
    assert [c[4] == scratch for c in calls[:3]] == [True] * 3 and scratch != plan.range_slot.data_ptr()       # a completion counts no event a second time
    # layer order: each launch reads what the one before it wrote
    names = [op[3] for op in plan.ops]
    assert [c[5] for c in calls[:3]] == [plan.ops[names.index(n)][2].inp for n in (LAYER1, LAYER2, LAYER3)]
    plan.regression_dim
    assert len(calls) == 5
    # a plan without the deep form issues what it always has
    calls.clear()
    plain = build(8, 402, 1333, env={'GPP_SPARSE_TOWER_DEPTH': '1'})
    plain.heads_stale = True
    plain.regression
    assert [c[0] for c in calls] == [512, 144, 36]
