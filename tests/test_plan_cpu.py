""" Plans built without a GPU: the model on the CPU device (hip.require_device patched, GPP_AUTOTUNE=0) builds every plan of the matrix
(helpers.plan_matrix: every plan switch x every type x several batches, the deeper ResNets, DenseNet, the latency plan, per-orientation
NMS, no NMS, a full-size frame, the regression tower's sparse and deep forms at 224 x 352, MobileNet, pose, audit and ragged plans).  What the plan builder asks of the library there is host code (FLOPs, workspace sizes, the split rule).
Each plan is checked for races between its streams, for descriptors the library would refuse, and for the host restatement of the split
rule (layers/conv.default_split) against the library's own. """
import ctypes
import os

import pytest
import torch

import helpers
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W

INNER = {R.OP_TAIL: ('conv3x3', 'conv1x1'), R.OP_BLOCK: ('conv1x1_a', 'conv3x3_b', 'conv1x1_c'), R.OP_CONV_PREACT: ('conv',)}


@pytest.fixture(scope='module')
def cpu_model():
    """ model_for(backbone, dtype, kwargs): one CPU model per configuration of the model, weights drawn once per backbone """
    weights, built = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def model_for(bb, dt, kw):
            key = (bb, dt, tuple(sorted(kw.items())))
            if key not in built:
                if bb not in weights:
                    weights[bb] = W.synthetic_weights(bb, 1234)
                built[key] = models.load_model(weights[bb], backbone_name=bb, dtype=dt, **kw)
            return built[key]
        yield model_for


def conv_descs(plan):
    """ every gpp_conv_desc of the plan, those inside fused and pre-activation launches included """
    for kind, _, desc, name, _ in plan.ops:
        if kind == R.OP_CONV:
            yield name, desc
        for field in INNER.get(kind, ()):
            yield name, hip.ConvDesc.from_address(getattr(desc, field))


@pytest.mark.parametrize('cfg', helpers.plan_matrix(), ids=helpers.plan_label)
def test_plan_is_race_free_and_every_descriptor_is_accepted(cfg, cpu_model, monkeypatch):
    bb, dt, kw, env, B, H, Wd = cfg
    kw = dict(kw)
    ragged = kw.pop('ragged', False)
    model = cpu_model(bb, dt, kw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model._plans.clear()
    plan = model.plan_for(B, H, Wd, 100, True, ragged=ragged)
    model._plans.clear()
    assert plan.check_stream_ordering() == []
    tiles, count = (ctypes.c_int * 64)(), ctypes.c_int(0)
    n = 0
    for name, d in conv_descs(plan):
        assert hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(d), tiles, 64, ctypes.byref(count)) == 0 and count.value > 0, name
        pixels = sum(d.groups[g].H_out * d.groups[g].W_out for g in range(d.n_groups))
        if model.plan_mode == 'throughput':
            assert C.default_split(d.KH, d.KW, d.C_in, d.C_out, pixels) == C.split_rule(d), name
        else:
            # the latency plan's descriptors carry their own factor, never below the rule's: the rule itself is asked with split_k = 0.
            # (default_split is needed before a descriptor exists -- the sparse heads' choice of form, the latency plan's floor -- so it
            # stays a restatement of the library's rule, held to it here)
            q = hip.ConvDesc.from_buffer_copy(d)
            q.split_k = 0
            assert C.default_split(d.KH, d.KW, d.C_in, d.C_out, pixels) == C.split_rule(q) <= C.split_rule(d), name
        n += 1
    # (a MobileNet backbone is 14 fused launches with no gpp_conv_desc: only the FPN's 8 layers and the heads' 13 carry one)
    assert n > (20 if model.mobilenet else 50)


def test_a_cpu_built_plan_never_reaches_a_kernel(cpu_model):
    model = cpu_model('resnet50', 'bf16', {})
    plan = model.plan_for(1, 96, 160, 100, True)
    for run in (lambda: model.run_op(plan, 0), lambda: model.run_plan(plan), lambda: model.capture(plan), lambda: model._autotune(plan)):
        with pytest.raises(hip.GppError):
            run()


PLAN_NAMES = ('StemDesc PoolDesc RaggedStemDesc RaggedPoolDesc ReluDesc DetectDesc CandidatePixelsDesc PollDesc PoseDesc PreactDesc '
              'DensePoolDesc PlanOp TailDesc BlockDesc '
              'OP_STEM OP_MAXPOOL OP_CONV OP_RELU OP_DETECT OP_POLL OP_TAIL OP_BLOCK OP_DETECT_CANDIDATES OP_DETECT_SELECT OP_DETECT_EMIT '
              'OP_DETECT_OSF OP_STEM_POOL OP_MAXPOOL_PAD OP_AVGPOOL OP_CONV_PREACT OP_MOBILENET_STEM OP_MOBILENET_BLOCK OP_POSE OP_ABSMAX '
              'OP_ABSMAX_CLEAR OP_STEM_RAGGED OP_STEM_POOL_RAGGED OP_MAXPOOL_RAGGED OP_DETECT_CANDIDATE_PIXELS DETECT_OPS OP_JOIN OP_SYNC '
              'PlanOptions block_form part_of TOWER_SLICES RANGE_AUDIT_THRESHOLD SPARSE_HEADS_MAX_SHARE audit_report SparseHeads Plan').split()


def test_the_plan_abi_lives_in_models_plan_under_the_names_retinanet_has_always_had():
    """ models/plan.py holds what a plan is (the mirrors of include/gpp.h, the op codes, PlanOptions, Plan ...); models/retinanet.py imports
    every name, so retinanet.StemDesc, retinanet.OP_CONV, retinanet.Plan ... are the same objects """
    from keras_retinanet_3D.models import plan as P
    assert len(PLAN_NAMES) == len(set(PLAN_NAMES)) == 14 + 28 + 9          # mirrors, op codes and flags, the rest
    for name in PLAN_NAMES:
        assert getattr(P, name) is getattr(R, name), name
    mirrors = [n for n in PLAN_NAMES if n.endswith('Desc') or n == 'PlanOp']
    assert len(mirrors) == 14 and all(issubclass(getattr(P, n), ctypes.Structure) and getattr(P, n).__module__ == P.__name__ for n in mirrors)
    assert P.Plan.__module__ == P.SparseHeads.__module__ == P.block_form.__module__ == P.__name__
