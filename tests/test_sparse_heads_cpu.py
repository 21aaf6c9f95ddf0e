""" Sparse head outputs in plans built without a GPU: the candidate pass writes the pixel lists on its side lane, the
guarded dense launch and the gathered launch of an output layer read them on the caller's stream -- Plan.check_stream_ordering must see
those reads and find the join that orders them, in the default plan, the classification-lane plan and the latency plan. """
import os

import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W


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


def gathered_ops(plan):
    return [i for i, (kind, _, desc, _, _) in enumerate(plan.ops) if kind == R.OP_CONV and desc.gather_rows]


# (B, H, W, what the plan is): the default plan, the plan with the classification tower on its own lane (B <= 2), the latency plan; 224 x 352 is
# the smallest size class at which the split rule leaves the regression output unsplit, so that both output layers are gathered
PLANS = [((4, 224, 352), {}, 'default'), ((2, 224, 352), {}, 'cls_lane'), ((1, 224, 352), {'plan': 'latency'}, 'latency')]


@pytest.mark.parametrize('shape,kw,what', PLANS, ids=[p[2] for p in PLANS])
def test_the_new_reads_are_ordered_and_a_missing_join_is_reported(build, shape, kw, what):
    plan = build(*shape, **kw)
    assert plan.side_lanes['cls_tower'] == (what in ('cls_lane', 'latency'))
    assert plan.sparse is not None and plan.check_stream_ordering() == []
    names = [op[3] for op in plan.ops]
    got = gathered_ops(plan)
    assert [names[i] for i in got] == ['pyramid_regression_ops', 'pyramid_regression_dim'] or what == 'latency'
    assert got and all(plan.ops[i][4] == 0.0 for i in got)               # the algorithmic FLOPs stay with the dense launch
    lists = names.index('filtered_detections/candidates')
    assert plan.ops[lists][0] == R.OP_DETECT_CANDIDATE_PIXELS and (plan.lanes[lists] >> 8) & 0xff in (1, 2)
    # the guarded dense launch stands directly in front of its gathered twin; it, or a launch between the lists and it, joins the candidates' lane
    first = got[0] - 1
    assert names[first] == names[got[0]] and plan.ops[first][2].guard and not plan.ops[first][2].gather_rows
    assert plan.ops[first][2].guard_value == 1 and plan.ops[got[0]][2].guard_value == 0
    joiner = next(i for i in range(lists + 1, len(plan.ops)) if plan.lanes[i] & R.OP_JOIN)
    assert joiner <= first and (what == 'latency' or joiner == first)
    saved = plan.lanes[joiner]
    plan.lanes[joiner] &= ~R.OP_JOIN
    bad = plan.check_stream_ordering()
    plan.lanes[joiner] = saved
    assert ('filtered_detections/candidates', names[first]) in bad
    assert plan.check_stream_ordering() == []


def test_the_switch_and_the_plans_that_keep_the_dense_launches(build):
    dense = build(4, 224, 352, env={'GPP_SPARSE_HEADS': '0'})
    sparse = build(4, 224, 352)
    assert dense.sparse is None and not gathered_ops(dense)
    assert all(op[0] != R.OP_DETECT_CANDIDATE_PIXELS for op in dense.ops)
    assert dense.flops == sparse.flops                                   # algorithmic work of the reference graph, either way
    assert len(sparse.ops) == len(dense.ops) + 2
    serial = build(4, 224, 352, env={'GPP_DECODE_OVERLAP': '0'})         # no candidate lists ahead of the towers: nothing to gather on
    assert serial.sparse is None and not gathered_ops(serial)
    small = build(2, 96, 160)                                            # the split rule splits the regression output here: it stays dense
    names = [op[3] for op in small.ops]
    assert [names[i] for i in gathered_ops(small)] == ['pyramid_regression_dim'] and small.check_stream_ordering() == []
    audit = build(2, 96, 160, range_audit=True)
    assert audit.sparse is None


def test_reading_a_head_tensor_completes_it_once(build, monkeypatch):
    plan = build(2, 96, 160)
    calls = []
    monkeypatch.setattr(hip.lib(), 'gpp_conv2d_igemm', lambda desc, stream: calls.append(desc._obj.guard) or 0, raising=False)
    monkeypatch.setattr(hip, 'stream_ptr', lambda: None)
    plan.regression, plan.regression_dim
    assert calls == []                                                   # nothing has run: nothing to complete
    plan.heads_stale = True                                              # (what run_plan leaves behind)
    plan.regression_dim
    assert len(calls) == len(plan.sparse.dense) == 1 and calls[0] is None and not plan.heads_stale
    plan.regression, plan.regression_dim
    assert len(calls) == 1
