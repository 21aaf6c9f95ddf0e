"""
The lower range of dtype='f16x3', audited (load_model(..., range_audit=True)) -- the mirror of
tests/test_range_reaction_gpu.py.

Below 2^-14 the (hi, lo) IEEE-half pair is a fixed-point number with a quantum of 2^-24.  An audit model measures the largest |x| of
every channel of every map an x3 convolution reads (gpp_channel_absmax), and a synchronous call whose run left the largest value of a
whole map below 2^-9 reacts as `on_range_event` says.

The weights that provoke it compute the SAME function as the seeded ones: bn2a_branch2a's (gamma, beta) x 2^-17 and res2a_branch2b's
kernel x 2^17 -- a ReLU commutes with a positive scale and powers of two are exact, so at float32 every tensor behind branch2b is
bit-identical to the unscaled network's, while the map between the two layers holds values around 1e-4.
"""
import numpy as np
import pytest
import torch

import helpers
from oracle import net_torch
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import ledger, synthetic

pytestmark = pytest.mark.gpu

SCALE = np.float32(2.0 ** 17)
LAYOUTS = {'f32': hip.GPP_ABSMAX_F32, 'split_f16': hip.GPP_ABSMAX_SPLIT_F16, 'split_bf16': hip.GPP_ABSMAX_SPLIT_BF16}
BIG = 8 * 101 * 334          # the pixels of the largest map of a B = 8 plan at 402 x 1333 (res2)


# ---------------------------------------------------------------- 6. the kernel against NumPy, bit for bit
def specials(rng, a, kinds):
    """ sprinkle the special values of `kinds` over `a` (in place; `a` may be a strided view) """
    for v in kinds:
        a.flat[rng.integers(0, a.size, size=max(1, a.size // 997))] = v


def make_f32(rng, rows, pitch, special=True):
    x = (rng.standard_normal((rows, pitch), dtype=np.float32) * np.exp2(rng.integers(-30, 12, size=(1, pitch))).astype(np.float32))
    if special:
        specials(rng, x.view(np.uint32), [0x80000000, 0x00000001, 0x807fffff, 0x00400000])       # -0 and subnormals
        specials(rng, x, [np.inf, -np.inf])
        x[:, ::7] = np.where(rng.random((rows, len(range(0, pitch, 7)))) < 0.02, np.float32(np.nan), x[:, ::7])       # NaN in some channels only
        x.view(np.uint32)[np.isnan(x) & (rng.random(x.shape) < 0.5)] = 0xffc00000                 # ... of either sign
    return x


def make_split(rng, rows, pitch, half, special=True):
    """ (rows, pitch) float32-sized elements whose every 32 are [32 halves hi | 32 halves lo]; returns (the raw array, its values) """
    chunks = pitch // 32
    v = rng.standard_normal((rows, chunks, 32)).astype(np.float32) * np.exp2(rng.integers(-22, 10, size=(1, chunks, 32))).astype(np.float32)
    if half == 'split_f16':
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
        raw = np.stack([hi.view(np.uint16), lo.view(np.uint16)], axis=2)                          # (rows, chunks, 2, 32)
        nan, inf = 0x7e00, 0x7c00
    else:
        hi = (v.view(np.uint32) >> 16).astype(np.uint16)
        lo = (((v - (hi.astype(np.uint32) << 16).view(np.float32)).view(np.uint32)) >> 16).astype(np.uint16)
        raw = np.stack([hi, lo], axis=2)
        nan, inf = 0x7fc0, 0x7f80
    if special:
        specials(rng, raw, [0x8000, 0x0001, 0x83ff, 0x0200])                                      # -0 and subnormal halves, hi or lo
        specials(rng, raw[:, :, 0, :], [inf, inf | 0x8000])
        sel = rng.random((rows, chunks, 8)) < 0.02
        raw[:, :, 0, ::4][sel] = np.where(rng.random(int(sel.sum())) < 0.5, nan, nan | 0x8000).astype(np.uint16)
    raw = np.ascontiguousarray(raw)
    if half == 'split_f16':
        vals = raw[:, :, 0, :].view(np.float16).astype(np.float32) + raw[:, :, 1, :].view(np.float16).astype(np.float32)
    else:
        vals = (raw[:, :, 0, :].astype(np.uint32) << 16).view(np.float32) + (raw[:, :, 1, :].astype(np.uint32) << 16).view(np.float32)
    return raw.reshape(rows, chunks * 64).view(np.float32).reshape(rows, pitch), vals.reshape(rows, pitch)


def device_absmax(layout, raw, M, C, pitch, c_off, parts=1, table_words=None):
    """ the kernel's table for rows [0, M) of `raw` (uploaded as it is, poison included), launched over `parts` row ranges """
    dev = torch.device('cuda')
    buf = torch.as_tensor(raw).to(dev).contiguous()
    words = table_words or C
    table = torch.full((words,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    hip.check(hip.lib().gpp_absmax_clear(hip.ptr(table), C, hip.stream_ptr()), 'gpp_absmax_clear')
    edges = [M * k // parts for k in range(parts + 1)]
    for a, b in zip(edges, edges[1:]):
        hip.channel_absmax(buf.view(-1)[a * pitch:], b - a, C, pitch, c_off, LAYOUTS[layout], table)
    torch.cuda.synchronize()
    return table.cpu().numpy().view(np.uint32)


def expected(vals, M, C, c_off):
    with np.errstate(invalid='ignore'):
        return np.abs(vals[:M, c_off:c_off + C]).max(axis=0).view(np.uint32)


F32_CASES = [(M, C, C, 0) for M in (1, 63, 64) for C in (8, 16, 36, 64, 256, 2048)] + \
            [(63, 36, 48, 8), (64, 36, 41, 3), (1, 8, 24, 16), (63, 16, 24, 4), (64, 64, 100, 36), (63, 256, 320, 32), (64, 2048, 2080, 32), (63, 7, 9, 1),
             (BIG, 64, 64, 0), (BIG, 8, 8, 0), (BIG // 8, 256, 256, 0), (BIG // 8, 36, 44, 4)]
SPLIT_CASES = [(M, C, C, 0) for M in (1, 63, 64) for C in (64, 256, 2048)] + \
              [(63, 32, 32, 0), (64, 64, 128, 32), (63, 256, 896, 512), (1, 128, 896, 768), (64, 2048, 2112, 64), (BIG, 64, 64, 0), (BIG // 8, 256, 256, 0)]


@pytest.mark.parametrize('M,C,pitch,c_off', F32_CASES)
def test_float32_rows_against_numpy(M, C, pitch, c_off):
    rng = np.random.default_rng(M * 131 + C)
    x = make_f32(rng, M + 2, pitch)
    poisoned = x.copy()
    poisoned[M:] = np.nan                                   # beyond M, and outside [c_off, c_off + C): never read into the result
    poisoned[:, :c_off] = np.nan
    poisoned[:, c_off + C:] = np.nan
    want = expected(x, M, C, c_off)
    got = device_absmax('f32', poisoned, M, C, pitch, c_off, table_words=C + 3)
    assert np.array_equal(got[:C], want) and np.all(got[C:] == 0x5a5a5a5a)
    if M > 1:
        assert np.array_equal(device_absmax('f32', poisoned, M, C, pitch, c_off, parts=2), want)       # two halves add up to the whole


@pytest.mark.parametrize('layout', ['split_f16', 'split_bf16'])
@pytest.mark.parametrize('M,C,pitch,c_off', SPLIT_CASES)
def test_split_rows_against_numpy(layout, M, C, pitch, c_off):
    rng = np.random.default_rng(M * 137 + C)
    raw, vals = make_split(rng, M + 2, pitch, layout)
    poisoned = raw.copy().view(np.uint16).reshape(M + 2, pitch // 32, 64)
    nan = 0x7e00 if layout == 'split_f16' else 0x7fc0
    poisoned[M:] = nan
    poisoned[:, :c_off // 32] = nan
    poisoned[:, (c_off + C) // 32:] = nan
    poisoned = poisoned.reshape(M + 2, 2 * pitch).view(np.float32)
    want = expected(vals, M, C, c_off)
    got = device_absmax(layout, poisoned, M, C, pitch, c_off, table_words=C + 3)
    assert np.array_equal(got[:C], want) and np.all(got[C:] == 0x5a5a5a5a)
    if M > 1:
        assert np.array_equal(device_absmax(layout, poisoned, M, C, pitch, c_off, parts=3), want)


def test_the_split_layouts_refuse_partial_channel_groups_on_the_device_too():
    buf = torch.zeros((64, 64), dtype=torch.float32, device='cuda')
    table = torch.zeros((64,), dtype=torch.int32, device='cuda')
    for C, pitch, c_off in ((36, 64, 0), (32, 64, 8)):
        with pytest.raises(hip.GppError, match='GPP_ERR_BAD_ARG'):
            hip.channel_absmax(buf, 64, C, pitch, c_off, hip.GPP_ABSMAX_SPLIT_F16, table)


# ---------------------------------------------------------------- the whole model
def inputs(B=2, H=96, Wd=160):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return [img, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]


def same(a, b):
    return all(helpers.bits_equal(x, y) if x.dtype.kind == 'f' else np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 8


def table_of(plan):
    torch.cuda.synchronize()
    return plan.audit_table.cpu().numpy().view(np.uint32)


def oracle_rows(trace, name):
    """ per-channel largest |x| of the oracle's layer(s) behind an audited map's name: the levels of a pyramid tensor merged """
    names = {'conv1+pool1': ['pool1']}.get(name, name.split('+'))
    got = [np.abs(y).reshape(-1, y.shape[-1]).max(axis=0) for (n, _), y in trace.items() if n in names]
    assert got, name
    return np.max(got, axis=0)


@pytest.mark.parametrize('H,Wd', [(96, 160), (75, 211)])
def test_every_row_is_the_maximum_of_its_own_map_and_of_the_layer_of_its_name(H, Wd):
    """ every row equals the maximum taken on the host from the plan's own buffer (exact), and -- to catch a row bound to the wrong map --
    agrees with the float32 oracle trace of the layer of its name within the project's f16 layer bar as DESIGN.md section 5.1 and
    tests/test_conv_gpu.py state it, |err| <= 2^-10 |ref| + 1e-3.  The absolute term belongs to that bar and is needed here: a channel
    maximum is one float32 activation, whose error against the oracle scales with the MAP's size (another summation order), not with its
    own.  Measured on the device: 0.012 of the bar at worst; without the absolute term the worst single channel reads 0.037 relative --
    2.229e-5 against 2.150e-5 in a map whose maximum is 14.0 (res5c_branch2a, channel 35), a difference of 6e-8 of the map's size. """
    B = 2
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3', range_audit=True)
    model.predict_on_batch(inputs(B, H, Wd))
    plan = model.plan_for(B, H, Wd, 100, True)
    table = table_of(plan)
    trace = net_torch.forward(W.synthetic_weights('resnet50', 1234), inputs(B, H, Wd)[0], 'resnet50', storage=None, trace=True)['trace']
    assert len(plan.audit_maps) == 70
    worst, worst_rel = (0.0, None), (0.0, None)
    for m in plan.audit_maps:
        first, n = m['row']
        host = torch.stack([f.read().abs().amax(dim=(0, 1, 2)) for f in m['fmaps']]).amax(dim=0).cpu().numpy()
        assert np.array_equal(table[first:first + n], host.view(np.uint32)), m['name']          # exact: the plan's own buffer
        want = oracle_rows(trace, m['name'])
        got = table[first:first + n].view(np.float32)
        # the project's f16 layer bar (tests/test_conv_gpu.py): |err| <= 2^-10 |ref| + 1e-3
        ratio = np.abs(got - want) / (2.0 ** -10 * want + 1e-3)
        c = int(ratio.argmax())
        worst = max(worst, (float(ratio[c]), m['name'], c, float(got[c]), float(want[c]), float(want.max())))
        rel = np.abs(got - want) / np.maximum(want, np.finfo(np.float32).tiny)
        c = int(rel.argmax())
        worst_rel = max(worst_rel, (float(rel[c]), m['name'], c, float(got[c]), float(want[c]), float(want.max())))
    print('largest |row - oracle| / |oracle| of a single channel: {:.3g} (map {}, channel {}: {:.6g} against {:.6g}; the map\'s maximum {:.4g})'.format(*worst_rel))
    print('largest |row - oracle| / (2^-10 |oracle| + 1e-3): {:.3g} (map {}, channel {}: {:.6g} against {:.6g}; the map\'s maximum {:.4g})'.format(*worst))
    # a row bound to the wrong map is off by tens of percent of the map's size in most channels: a binding check, not a precision claim
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize('spec', ['synthetic:1234', 'synthetic:1234:trained'])
@pytest.mark.parametrize('B', [2, 3])
def test_sane_weights_the_audit_model_returns_the_bytes_of_the_ordinary_one(spec, B):
    plain = models.load_model(spec, backbone_name='resnet50', dtype='f16x3')
    audit = models.load_model(spec, backbone_name='resnet50', dtype='f16x3', range_audit=True)
    x = inputs(B)
    want, got = plain.predict_on_batch(x), audit.predict_on_batch(x)
    assert same(got, want) and int((got[2] > 0.05).sum()) > 0
    report = audit.range_audit()
    assert report == audit.last_range_audit and len(report) == 70 and not any(r['flagged'] for r in report)
    assert min(r['absmax'] for r in report) >= 256 * R.RANGE_AUDIT_THRESHOLD        # (tests/test_range_audit_cpu.py: 3000 x at float32)
    assert audit.range_fallbacks == 0 and audit.small_magnitude_events == 0 and audit._twin is None and plain.range_fallbacks == 0
    plan = audit.plan_for(B, 96, 160, 100, True)
    assert not any(op[0] in (R.OP_BLOCK, R.OP_TAIL) for op in plan.ops) and any(op[0] == R.OP_BLOCK for op in plain.plan_for(B, 96, 160, 100, True).ops)
    if B == 2:
        # the replayed graph clears and refills the table
        first = table_of(plan).copy()
        audit.capture(plan)
        plan.audit_table.fill_(0x7fffffff)
        audit.run_plan(plan)
        assert np.array_equal(table_of(plan), first) and same(audit.fetch(plan), want)
        plan.audit_table.fill_(0x7fffffff)
        assert same(audit.predict_on_batch(x), want) and np.array_equal(table_of(plan), first)


def mirror_weights(small=('bn2a_branch2a/gamma', 'bn2a_branch2a/beta'), large=('res2a_branch2b/kernel',)):
    w = dict(W.synthetic_weights('resnet50', 1234))
    for k in small:
        w[k] = w[k] / SCALE
    for k in large:
        w[k] = w[k] * SCALE
    return w


MIRRORS = {'res2a_branch2a': mirror_weights(),
           'pyramid_regression_1': mirror_weights(('pyramid_regression_1/kernel', 'pyramid_regression_1/bias'), ('pyramid_regression_2/kernel',))}


@pytest.fixture(scope='module')
def f32_of_the_base_weights():
    return models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())


@pytest.mark.parametrize('name', sorted(MIRRORS))
def test_a_call_whose_map_sits_below_the_half_pairs_resolution_returns_the_float32_result(name, f32_of_the_base_weights):
    """ the mirror of test_a_call_whose_activations_leave_the_half_range_returns_the_float32_result """
    w = MIRRORS[name]
    model = models.load_model(w, backbone_name='resnet50', dtype='f16x3', range_audit=True)          # on_range_event='f32' is the default
    assert model.range_fallbacks == 0 and model.small_magnitude_events == 0
    out = model.predict_on_batch(inputs())
    flagged = [r for r in model.last_range_audit if r['flagged']]
    assert [r['name'] for r in flagged] == [name] and 0 < flagged[0]['absmax'] < R.RANGE_AUDIT_THRESHOLD and flagged[0]['bits'] < 16
    assert model.range_fallbacks == 1 and model.small_magnitude_events == 1 and model.x3_range_events() == 0
    want = models.load_model(w, backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())
    assert same(out, want)                                    # byte for byte what dtype='f32' returns for these weights
    assert same(out, f32_of_the_base_weights)                 # ... which is what the unscaled network returns at float32 (exact scaling)
    assert int((out[2] > 0.05).sum()) > 0
    again = model.predict_on_batch(inputs())                  # every further call is watched too
    assert model.range_fallbacks == 2 and model.small_magnitude_events == 2 and same(again, want)


def test_raise_names_the_map_and_ignore_returns_the_damaged_result(f32_of_the_base_weights):
    w = MIRRORS['res2a_branch2a']
    strict = models.load_model(w, backbone_name='resnet50', dtype='f16x3', range_audit=True, on_range_event='raise')
    with pytest.raises(hip.GppError, match=r'res2a_branch2a \(read by res2a_branch2b; max [0-9.e-]+\)'):
        strict.predict_on_batch(inputs())
    assert strict.range_fallbacks == 1
    loose = models.load_model(w, backbone_name='resnet50', dtype='f16x3', range_audit=True, on_range_event='ignore')
    got = loose.predict_on_batch(inputs())                    # the coarsely stored map goes through: a finite, plausible, different answer
    assert loose.range_fallbacks == 0 and loose.small_magnitude_events == 1 and loose._twin is None
    assert [r['name'] for r in loose.last_range_audit if r['flagged']] == ['res2a_branch2a']
    assert not same(got, f32_of_the_base_weights)
    # for the record, not a bar (profiles/range_audit/README.md): what the UNWATCHED model returns for these weights against float32
    unwatched = models.load_model(w, backbone_name='resnet50', dtype='f16x3')
    u = unwatched.predict_on_batch(inputs())
    assert unwatched.range_fallbacks == 0 and same(u, got)    # nothing else in the tree reacts, and the audit changed no byte
    ref = models.load_model(w, backbone_name='resnet50', dtype='f32')
    r = ref.predict_on_batch(inputs())
    pu, pr = unwatched.plan_for(2, 96, 160, 100, True), ref.plan_for(2, 96, 160, 100, True)
    led = ledger.parity_ledger(r, pr.anchor_index.cpu().numpy(), pr.best_index.cpu().numpy(), u, pu.anchor_index.cpu().numpy(), pu.best_index.cpu().numpy())
    reg = np.abs(pu.regression.cpu().numpy() - pr.regression.cpu().numpy()).max()
    print('unwatched f16x3 on the mirror weights against float32: largest change of a regression output {:.3g}; ledger {}'.format(
        reg, {k: led[k] for k in sorted(led) if k in ('set_differences', 'common', 'max_corner_dev_m_within_100m', 'max_keypoint_rel_dev', 'same_plane')}))


def test_the_pose_calls_react_too():
    w = MIRRORS['res2a_branch2a']
    model = models.load_model(w, backbone_name='resnet50', dtype='f16x3', range_audit=True, pose=True)
    rows, counts = model.predict_poses_on_batch(inputs(), 1.0, (96, 160))
    want = models.load_model(w, backbone_name='resnet50', dtype='f32', pose=True).predict_poses_on_batch(inputs(), 1.0, (96, 160))
    assert model.range_fallbacks == 1 and model.small_magnitude_events == 1
    assert helpers.bits_equal(rows, want[0]) and np.array_equal(counts, want[1])
    model.on_range_event = 'raise'
    with pytest.raises(hip.GppError, match='res2a_branch2a'):
        model.predict_poses_on_batch(inputs(), 1.0, (96, 160))


@pytest.mark.parametrize('bb,unobserved', [('densenet121', 61), ('mobilenet224_1.0', 13)])
def test_densenet_and_mobilenet_audit_models_equal_their_twins_and_list_what_they_cannot_see(bb, unobserved):
    x = inputs()
    plain = models.load_model('synthetic:1234', backbone_name=bb, dtype='f16x3')
    audit = models.load_model('synthetic:1234', backbone_name=bb, dtype='f16x3', range_audit=True)
    assert same(audit.predict_on_batch(x), plain.predict_on_batch(x))
    report, unseen = audit.range_audit(), audit.range_audit_unobserved()
    assert len(unseen) == unobserved and all(u['reason'] and u['consumers'] for u in unseen)
    assert not any(r['flagged'] for r in report) and audit.range_fallbacks == 0
    plan = audit.plan_for(2, 96, 160, 100, True)
    table = table_of(plan)
    for m in plan.audit_maps:                                 # float32 rows with a pitch, channel slices of a concatenation buffer
        first, n = m['row']
        host = torch.stack([f.read().abs().amax(dim=(0, 1, 2)) for f in m['fmaps']]).amax(dim=0).cpu().numpy()
        assert np.array_equal(table[first:first + n], host.view(np.uint32)), m['name']
    assert {m['layout'] for m in plan.audit_maps} == {'f32', 'split_f16'}
