""" The range audit of dtype='f16x3' (load_model(..., range_audit=True)), the parts that need no GPU:
the report and its criterion on hand-made tables, audit plans built on the CPU device (race-free, no fused launch, every x3 activation
operand of every conv descriptor inside an audited map or listed as unobserved), the untouched plans of every other model, the
refusals, the library's argument checks, and -- with the float32 oracle alone -- how far the weights of the GPU tests sit from the
threshold. """
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import net_torch
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W

THR = 2.0 ** -9


def bits(values):
    return np.asarray(values, np.float32).view(np.uint32)


def report_of(*rows):
    maps, first = [], 0
    for i, row in enumerate(rows):
        maps.append({'name': 'map{}'.format(i), 'consumers': ['conv{}'.format(i)], 'channels': len(row), 'row': (first, len(row))})
        first += len(row)
    return R.audit_report(maps, np.concatenate([bits(r) for r in rows]))


# ---------------------------------------------------------------- 1. the report
def test_the_threshold_is_two_to_the_minus_nine_and_exclusive():
    assert R.RANGE_AUDIT_THRESHOLD == THR
    below = np.nextafter(np.float32(THR), np.float32(0))
    at, under, tiny = report_of([THR, 1e-6, 0.0], [below, 1e-6], [2.0 ** -24])
    assert not at['flagged'] and under['flagged'] and tiny['flagged']
    assert at['absmax'] == THR and under['absmax'] == float(below)
    assert (at['bits'], under['bits'], tiny['bits']) == (15, 14, 0)          # 2^-9 / 2^-24 = 2^15: the 16th bit is the first one kept whole


def test_dead_channels_all_zero_maps_and_small_channels():
    mixed, dead = report_of([0.0, 3.0, 1e-4, 0.5, 0.0, 2.0 ** -10], [0.0, 0.0, 0.0, 0.0])
    assert (mixed['channels'], mixed['live'], mixed['small_channels']) == (6, 4, 2) and not mixed['flagged']       # tiny channels inform, the map decides
    assert mixed['absmax'] == 3.0 and mixed['absmax_min_live'] == float(np.float32(1e-4)) and mixed['absmax_median_live'] == pytest.approx(0.25049, abs=1e-4)
    assert mixed['bits'] == 22                                               # capped: 3 / 2^-24 has 25 bits, a half pair keeps 22
    assert (dead['live'], dead['absmax'], dead['flagged'], dead['bits'], dead['absmax_min_live']) == (0, 0.0, False, None, None)
    assert mixed['name'] == 'map0' and mixed['consumers'] == ['conv0']


def test_a_nan_row_is_not_this_guards_business():
    nan, inf = report_of([1e-5, np.nan, 1e-4], [np.inf, 1.0])
    assert np.isnan(nan['absmax']) and not nan['flagged'] and nan['live'] == 3 and nan['small_channels'] == 2 and nan['bits'] is None
    assert inf['absmax'] == np.inf and not inf['flagged'] and inf['bits'] == 22


# ---------------------------------------------------------------- 2. audit plans on the CPU device
INNER = {R.OP_TAIL: ('conv3x3', 'conv1x1'), R.OP_BLOCK: ('conv1x1_a', 'conv3x3_b', 'conv1x1_c'), R.OP_CONV_PREACT: ('conv',)}


@pytest.fixture(scope='module')
def cpu_model():
    """ model_for(backbone, dtype, kwargs): one CPU model per configuration of the model, weights drawn once per backbone
    (as tests/test_plan_cpu.py builds its models) """
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


AUDIT_PLANS = [('resnet50', {}, 1), ('resnet50', {}, 2), ('resnet50', {}, 8), ('resnet101', {}, 1), ('resnet101', {}, 2), ('resnet101', {}, 8),
               ('resnet50', {'plan': 'latency'}, 1), ('densenet121', {}, 2), ('mobilenet224_1.0', {}, 2)]


@pytest.mark.parametrize('bb,kw,B', AUDIT_PLANS, ids=lambda v: str(v))
def test_audit_plan_is_race_free_unfused_and_covers_every_x3_operand(bb, kw, B, cpu_model):
    model = cpu_model(bb, 'f16x3', dict(kw, range_audit=True))
    model._plans.clear()
    plan = model.plan_for(B, 200, 333, 100, True)
    model._plans.clear()
    assert plan.check_stream_ordering() == []
    kinds = [op[0] for op in plan.ops]
    assert R.OP_BLOCK not in kinds and R.OP_TAIL not in kinds
    assert kinds[0] == R.OP_ABSMAX_CLEAR and kinds.count(R.OP_ABSMAX_CLEAR) == 1 and kinds.count(R.OP_ABSMAX) >= len(plan.audit_maps)
    observed = [m['extent'] for m in plan.audit_maps]
    unobserved = [u['extent'] for u in plan.audit_unobserved if u['extent']]
    preact = {name for kind, _, _, name, _ in plan.ops if kind == R.OP_CONV_PREACT}
    n = 0
    for name, d in conv_descs(plan):                       # from the descriptors themselves, not from the builder's bookkeeping
        assert d.dtype == hip.GPP_F16X3
        for g in range(d.n_groups):
            p = d.inp + d.groups[g].in_off * 4
            where = unobserved if name in preact else observed
            assert any(lo <= p < hi for lo, hi in where), (name, g)
            n += 1
    assert n > 50
    # every map's row of the table is written by at least one launch, inside the table, and rows do not overlap
    t0, t1 = plan.audit_table.data_ptr(), plan.audit_table.data_ptr() + 4 * plan.audit_table.numel()
    rows = sorted(m['row'] for m in plan.audit_maps)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(rows, rows[1:])) and rows[-1][0] + rows[-1][1] == plan.audit_table.numel()
    written = np.zeros(plan.audit_table.numel(), bool)
    for kind, _, d, _, _ in plan.ops:
        if kind == R.OP_ABSMAX:
            assert t0 <= d.out and d.out + 4 * d.C <= t1 and d.M > 0 and d.reserved == 0
            written[(d.out - t0) // 4:(d.out - t0) // 4 + d.C] = True
    assert written.all()
    for m in plan.audit_maps:
        assert m['name'] and m['consumers'] and m['layout'] in ('f32', 'split_f16')
    if bb.startswith('densenet'):
        assert len(plan.audit_unobserved) == len(preact) and any(m['consumers'] == ['conv2_block1_2_conv'] and m['channels'] == 128 for m in plan.audit_maps)
    elif bb.startswith('mobilenet'):
        assert [u['name'] for u in plan.audit_unobserved] == ['conv_dw_{}'.format(i) for i in range(1, 14)]
    else:
        assert plan.audit_unobserved == []
        names = [m['name'] for m in plan.audit_maps]
        for want in ('conv1+pool1', 'res2a_branch2a', 'res2a_branch2b', 'res2a_branch1', 'res5c_branch2c', 'C5_reduced', 'C6_relu', 'P3+P4+P5+P6+P7',
                     'pyramid_regression_0', 'pyramid_classification_0', 'pyramid_regression_dim_0', 'pyramid_regression_3', 'pyramid_classification_3'):
            assert names.count(want) == 1, want


# ---------------------------------------------------------------- 3. every other model is what it was
def test_a_model_without_the_flag_has_no_audit_op_and_keeps_its_tune_key(cpu_model):
    plain, audit = cpu_model('resnet50', 'f16x3', {}), cpu_model('resnet50', 'f16x3', {'range_audit': True})
    plan = plain.plan_for(2, 200, 333, 100, True)
    assert not any(op[0] in (R.OP_ABSMAX, R.OP_ABSMAX_CLEAR) for op in plan.ops)
    assert plan.audit_table is None and plan.audit_maps == [] and all(a == [] for a in plan.atomic)
    assert R.OP_BLOCK in [op[0] for op in plan.ops]                                     # (the fused forms are still what an ordinary plan runs)
    key = plain._plan_options(2).tune_key
    assert key == 'x3split=2;fuse=64,128/64,128;plan=throughput'                        # the string it was before the audit existed
    assert audit._plan_options(2).tune_key == key + ';audit'
    with pytest.raises(hip.GppError, match='range_audit=True'):
        plain.range_audit()


# ---------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize('dtype', ['bf16x3', 'f32', 'f16', 'bf16'])
def test_other_types_are_refused(dtype, cpu_model):
    with pytest.raises(ValueError, match='f16x3'):
        cpu_model('resnet50', dtype, {'range_audit': True})


def test_pipeline_and_sharded_model_refuse_an_audit_model(cpu_model):
    from keras_retinanet_3D.utils import distributed as D
    from keras_retinanet_3D.utils.pipeline import FramePipeline
    model = cpu_model('resnet50', 'f16x3', {'range_audit': True})
    with pytest.raises(ValueError, match='range_audit'):
        FramePipeline(model)
    with pytest.raises(ValueError, match='range_audit'):
        D.ShardedModel(model)


def test_the_entry_points_check_their_arguments_without_a_device():
    lib = hip.lib()
    IN, OUT = 0x10000, 0x20000                      # never dereferenced: every case below returns before a launch

    def rc(inp=IN, out=OUT, M=16, pitch=64, C=64, c_off=0, layout=hip.GPP_ABSMAX_F32, reserved=0):
        d = hip.AbsmaxDesc(inp, out, M, pitch, C, c_off, layout, reserved)
        return lib.gpp_channel_absmax(ctypes.byref(d), None)
    bad = -1
    assert lib.gpp_channel_absmax(None, None) == bad
    assert rc(inp=None) == bad and rc(out=None) == bad
    assert rc(C=0) == bad and rc(C=-4) == bad and rc(M=-1) == bad
    assert rc(pitch=32) == bad and rc(pitch=64, C=48, c_off=32) == bad and rc(c_off=-1) == bad
    assert rc(layout=0) == bad and rc(layout=4) == bad and rc(reserved=1) == bad
    for split in (hip.GPP_ABSMAX_SPLIT_F16, hip.GPP_ABSMAX_SPLIT_BF16):
        assert rc(layout=split, C=36, pitch=64) == bad and rc(layout=split, C=32, pitch=72) == bad and rc(layout=split, C=32, c_off=8) == bad
        assert rc(layout=split, inp=IN + 64) == -3                           # GPP_ERR_ALIGN: whole 128-byte channel groups
        assert rc(layout=split, M=0) == 0
    assert rc(inp=IN + 2) == -3
    assert rc(M=0) == 0 and rc(M=0, C=8, pitch=8) == 0                       # nothing to read: nothing launched
    assert lib.gpp_absmax_clear(None, 4, None) == bad and lib.gpp_absmax_clear(OUT, -1, None) == bad and lib.gpp_absmax_clear(OUT, 0, None) == 0


# ---------------------------------------------------------------- 5. what the GPU tests rest on
def conv_operand_maxima(weights, images):
    """ {map: largest |x|} of every map a convolution reads, from the float32 oracle's trace; the levels of a pyramid tensor merged """
    trace = net_torch.forward(weights, images, 'resnet50', storage=None, trace=True)['trace']
    heads = ('pyramid_regression_op', 'pyramid_regression_dim', 'pyramid_classification')
    out = {}
    for (name, _), y in trace.items():
        if name == 'conv1' or name in heads[1:] or name.startswith(heads[0]):       # conv1 feeds the pool; head outputs are nobody's operand
            continue
        name = 'P3+P4+P5+P6+P7' if name in ('P3', 'P4', 'P5', 'P6', 'P7') else name
        out[name] = max(out.get(name, 0.0), float(np.abs(y).max()))
    return out


@pytest.mark.parametrize('spec', ['synthetic:1234', 'synthetic:1234:trained'])
@pytest.mark.parametrize('shape', [(2, 96, 160), (3, 75, 211)])
def test_sane_weights_sit_far_above_the_threshold_at_float32(spec, shape):
    """ "a sane model is never flagged" (tests/test_range_audit_gpu.py) is not decided by float32 noise: the smallest conv-operand map
    maximum of the float32 oracle is at least 256 x the threshold for the weights and frames those tests use """
    seed, family = W.parse_synthetic(spec)
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=shape + (3,)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
    maxima = conv_operand_maxima(W.synthetic_weights('resnet50', seed, family), img)
    assert len(maxima) == 70                    # the 70 rows of a ResNet-50 audit plan (pool1 here is its conv1+pool1)
    name = min(maxima, key=maxima.get)
    print('smallest conv-operand map maximum: {} = {:.4g} ({:.0f} x the threshold)'.format(name, maxima[name], maxima[name] / THR))
    assert maxima[name] >= 256 * THR, (name, maxima[name])


# ---------------------------------------------------------------- the command line
def test_run_network_refuses_the_audit_for_other_types_and_keeps_the_smallest_report_per_map(capsys):
    from keras_retinanet_3D.bin import run_network
    argv = ['synthetic:1.h5', 'img', 'calib', 'planes.mat', 'out', '--range-audit']
    assert run_network.parse_args(argv).range_audit and not run_network.parse_args(argv[:-1]).range_audit
    with pytest.raises(SystemExit):
        run_network.parse_args(argv + ['--dtype', 'bf16x3'])
    assert 'f16x3' in capsys.readouterr().err

    class Model(object):
        audit = True
    acc, model = {}, Model()
    for values in ([3.0, 0.5], [2.0, 0.75], [np.nan, 0.6]):
        model.last_range_audit = report_of([values[0]], [values[1]])
        run_network.keep_smallest(acc, model)
    assert np.isnan(acc['map0']['absmax']) and acc['map1']['absmax'] == 0.5       # the minimum over the calls; a NaN stays
