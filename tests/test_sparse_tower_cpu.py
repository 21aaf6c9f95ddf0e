""" Sparse regression tower in plans built without a GPU: pyramid_regression_3 stays ONE op with the tower's tag and
the algorithmic FLOPs, reads the dilated lists the candidate pass writes on its side lane -- Plan.check_stream_ordering must see those
reads and find the join in front of the op --, and only plans whose dense launch fields more than a round of workgroups take the form. """
import os

import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W

TOWER = 'pyramid_regression_3'


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


def tower_ops(plan):
    return [i for i, (kind, _, desc, _, _) in enumerate(plan.ops) if kind == R.OP_CONV and desc.tower_rows]


@pytest.fixture(scope='module')
def flagship(build):
    return build(8, 402, 1333), build(8, 402, 1333, env={'GPP_SPARSE_TOWER': '0'})


def test_the_flagship_plan_orders_the_reads_of_the_dilated_lists(flagship):
    plan, _ = flagship
    sp = plan.sparse
    assert sp is not None and sp.tower_rows is not None and plan.check_stream_ordering() == []
    names = [op[3] for op in plan.ops]
    got = tower_ops(plan)
    assert [names[i] for i in got] == [TOWER] and names.count(TOWER) == 1
    kind, tag, desc, _, flops = plan.ops[got[0]]
    assert kind == R.OP_CONV and tag == 1 and flops > 0 and not desc.gather_rows and not desc.guard
    assert desc.tower_rows == sp.tower_rows.data_ptr() and desc.tower_counts == sp.tower_counts.data_ptr() and desc.tower_flag == sp.tower_flag.data_ptr()
    assert sp.tower == [desc] and len(sp.dense) == 2
    assert [n for _, t, _, n, _ in plan.ops if t == 1] == ['pyramid_regression_1', 'pyramid_regression_2', TOWER]
    # the candidate pass writes both sets of lists; the tower op is the first JOIN behind it
    lists = names.index('filtered_detections/candidates')
    assert plan.ops[lists][0] == R.OP_DETECT_CANDIDATE_PIXELS and (plan.lanes[lists] >> 8) & 0xff == 1
    pl = plan.ops[lists][2].lists
    assert pl.dilated_rows == sp.tower_rows.data_ptr() and pl.dilated_flag == sp.tower_flag.data_ptr() and pl.dilated_max_rows == sp.tower_max_rows
    assert list(pl.level_width)[:5] == [plan.features['P{}'.format(i + 3)].W for i in range(5)]
    joiner = next(i for i in range(lists + 1, len(plan.ops)) if plan.lanes[i] & R.OP_JOIN)
    assert joiner == got[0]
    saved = plan.lanes[joiner]
    plan.lanes[joiner] &= ~R.OP_JOIN
    bad = plan.check_stream_ordering()
    plan.lanes[joiner] = saved
    assert ('filtered_detections/candidates', TOWER) in bad
    assert plan.check_stream_ordering() == []


def test_the_switch_changes_neither_the_op_count_nor_the_flops(flagship):
    plan, off = flagship
    assert off.sparse is not None and off.sparse.tower_rows is None and not tower_ops(off) and off.sparse.tower == []
    assert len(plan.ops) == len(off.ops) and plan.flops == off.flops
    assert [op[3] for op in plan.ops] == [op[3] for op in off.ops] and [op[4] for op in plan.ops] == [op[4] for op in off.ops]
    assert off.check_stream_ordering() == []


@pytest.mark.parametrize('shape', [(4, 224, 352), (2, 96, 160)])
def test_plans_below_one_round_carry_no_list(build, shape):
    plan = build(*shape)
    assert plan.sparse is not None and plan.sparse.tower_rows is None and not tower_ops(plan) and plan.sparse.tower == []
    forced = build(*shape, env={'GPP_SPARSE_TOWER_MIN_ROUNDS': '0'})
    # (2 x 96 x 160: the split rule splits the regression output, which stays dense and reads every row -- no form to take)
    assert bool(tower_ops(forced)) == (shape == (4, 224, 352)) and forced.check_stream_ordering() == []


def test_reading_a_head_tensor_runs_the_tower_layer_dense_first(build, monkeypatch):
    plan = build(4, 224, 352, env={'GPP_SPARSE_TOWER_MIN_ROUNDS': '0'})
    calls = []
    monkeypatch.setattr(hip.lib(), 'gpp_conv2d_igemm',
                        lambda desc, stream: calls.append((desc._obj.C_out, desc._obj.tower_rows, desc._obj.guard, desc._obj.range_counter)) or 0, raising=False)
    monkeypatch.setattr(hip, 'stream_ptr', lambda: None)
    plan.heads_stale = True
    plan.regression
    assert [c[0] for c in calls] == [512, 144, 36] and all(c[1] is None and c[2] is None for c in calls)
    assert calls[0][3] == plan.sparse.range_scratch.data_ptr() != plan.range_slot.data_ptr()      # a completion counts no event a second time
    plan.regression_dim
    assert len(calls) == 3
