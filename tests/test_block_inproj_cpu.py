""" The fused projection block in plans built without a GPU: the flagship plan runs res2a as ONE op per half batch with
no res2a_branch1 launch and unchanged FLOPs; every plan that misses a condition of the rule keeps the parent's ops. """
import ctypes
import os

import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import plan as P
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W

FUSED, BRANCH1, BRANCH2A, TAIL = 'res2a_branch2a+2b+2c', 'res2a_branch1', 'res2a_branch2a', 'res2a_branch2b+2c'


@pytest.fixture(scope='module')
def build():
    weights = W.synthetic_weights('resnet50', 1234)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def plan_for(B, H, Wd, env=(), dtype='f16x3', **kw):
            for k, v in dict(env).items():
                mp.setenv(k, v)
            try:
                return models.load_model(weights, backbone_name='resnet50', dtype=dtype, **kw).plan_for(B, H, Wd, 100, True)
            finally:
                for k in dict(env):
                    mp.delenv(k)
        yield plan_for


def names_of(plan):
    return [op[3] for op in plan.ops]


def test_the_flagship_plan_runs_res2a_as_one_op_per_half_batch(build):
    on, off = build(8, 402, 1333), build(8, 402, 1333, env={'GPP_FUSE_BLOCK_INPROJ': '0'})
    names = names_of(on)
    assert names.count(FUSED) == 2 and BRANCH1 not in names and BRANCH2A not in names and TAIL not in names
    assert names_of(off).count(BRANCH1) == 2 and names_of(off).count(BRANCH2A) == 2 and FUSED not in names_of(off)
    assert [n for n in names if not n.startswith('res2a_')] == [n for n in names_of(off) if not n.startswith('res2a_')]
    assert on.flops == off.flops
    assert on.check_stream_ordering() == [] and off.check_stream_ordering() == []
    for index, (kind, _, desc, name, _) in enumerate(on.ops):
        if name != FUSED:
            continue
        assert kind == R.OP_BLOCK and isinstance(desc, P.BlockProjDesc) and desc.form == 1 and desc.conv1x1_proj
        inputs, outputs, residuals = on.op_io[index]
        assert residuals is None and len(inputs) == 1 and len(outputs) == 1 and inputs[0].B == 4 and not inputs[0].split
        a, c, p = (hip.ConvDesc.from_address(getattr(desc, f)) for f in ('conv1x1_a', 'conv1x1_c', 'conv1x1_proj'))
        assert p.inp == a.inp and p.in_pitch == a.in_pitch and p.groups[0].in_off == a.groups[0].in_off and p.x3_split == a.x3_split == 2
        assert not c.residual and c.x3_split == 3 and p.C_out == c.C_out == 256 and not p.relu


def test_the_rule_is_one_of_layer_map_size_and_batch_part():
    assert P.inproj_rounds(4, 101, 334) == 4 * 13 * 24 / 512.0 > 1.0            # the flagship's half batches: 1 248 tiles
    assert P.inproj_rounds(2, 50, 84) < 1.0 and P.inproj_rounds(1, 50, 84) < 1.0


@pytest.mark.parametrize('shape,env,kw', [
    ((3, 200, 333), {}, {}),                                   # 42-84 tiles per part: below one round
    ((8, 402, 1333), {}, {'range_audit': True}),
    ((8, 402, 1333), {}, {'dtype': 'bf16'}),
    ((8, 402, 1333), {}, {'dtype': 'f32'}),
    ((8, 402, 1333), {'GPP_FUSE_BLOCK': ''}, {}),
    ((8, 402, 1333), {'GPP_FUSE_BLOCK_INPROJ': '0'}, {}),
], ids=['small', 'audit', 'bf16', 'f32', 'no-fused-blocks', 'switch-off'])
def test_plans_that_miss_a_condition_keep_the_parents_ops(build, shape, env, kw):
    """ the parent's res2a: branch2a and branch1 as launches of their own -- and the very same op names whether the switch is on or off """
    plan = build(*shape, env=env, **kw)
    names = names_of(plan)
    assert FUSED not in names and names.count(BRANCH1) == names.count(BRANCH2A) >= 1
    off = build(*shape, env=dict(env, GPP_FUSE_BLOCK_INPROJ='0'), **kw)
    assert names == names_of(off) and plan.flops == off.flops
    assert all(not isinstance(op[2], P.BlockProjDesc) for op in plan.ops)
    assert ctypes.sizeof(P.BlockProjDesc) == ctypes.sizeof(P.BlockDesc) + 8
