"""
The stem, pooling and ReLU kernels (csrc/stem.hip, csrc/stem_kernels.h, csrc/densenet.hip) at their edges, against the float64 / raw-word
oracle of tests/stem_oracle.py (plain NumPy; tests/test_stem_oracle_cpu.py checks it against torch and shows the operand parts of the
bounds used here with no kernel involved).  Every test names the branch or boundary it exists for: tile edge, stride loop, padding value,
half-word pattern.  NaN inputs are out of scope (fmaxf drops a NaN); nothing here asserts on one.

The stem bounds (u = 2^-24, the float32 unit roundoff; mag = sum |x||w| of the output, from the oracle):
  * float32 kernel: 147 fmaf roundings and the bias addition, each relative to a partial sum that never exceeds mag + |b|:
        acc = 149 u (mag + |b|);      stored value: + u_out |ref| (u_out = 2^-8 bf16, 2^-11 f16, 0 float32), + 2^-25 for f16 (half its
        smallest subnormal); the rounding acts on the computed value, so acc enters as acc (1 + u_out)
  * MFMA kernel: x and w rounded to f16, 2^-11 each: 2^-10 mag; + the same acc and output terms
  * x3 kernel: operands kept as hi + lo (2^-22 each), lo * lo dropped (2^-22): 3 * 2^-22 mag = 12 u mag; 3 * 147 products + the scale
    multiplication + the bias addition accumulated in float32: 443 u mag;  together 455 u mag, + 1e-5 |ref|.  That magnitude bound
    holds on every shape; maps of 256 pixels and more also meet the project's own bars of test_x3_stem_matches_float64
    (|err| <= 1e-5 |ref| + 2e-6 sqrt(147) rms_c, rms(err) <= 5e-7 rms_c + 1e-8), which are about ten times tighter but mean nothing
    on a map of one pixel, where there is no rms to speak of.
"""
import ctypes

import numpy as np
import pytest
import torch

import stem_oracle as SO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')
TDT = {hip.GPP_BF16: torch.bfloat16, hip.GPP_F16: torch.float16, hip.GPP_F32: torch.float32}
U_OUT = {hip.GPP_BF16: 2.0 ** -8, hip.GPP_F16: 2.0 ** -11, hip.GPP_F32: 0.0}
SUB_OUT = {hip.GPP_BF16: 0.0, hip.GPP_F16: 2.0 ** -25, hip.GPP_F32: 0.0}
NAMES = {hip.GPP_BF16: 'bf16', hip.GPP_F16: 'f16', hip.GPP_F32: 'f32', hip.GPP_BF16X3: 'bf16x3', hip.GPP_F16X3: 'f16x3'}


def dev():
    return torch.device('cuda')


def put(a):
    return torch.from_numpy(np.array(a, order='C')).to(dev())          # (a copy: the shared inputs are read-only arrays)


def conv_shape(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


# -------------------------------------------------------------------------------------------------------------- stems
_REFS = {}


def stem_refs(B, H, W):
    """ per shape, computed once and left unchanged: the inputs on the device, and for both kernels (plain, four decades) the float64
    reference, its magnitude sum |x||w| and the pre-activation sum """
    key = (B, H, W)
    if key not in _REFS:
        x, k, k_dec, bias = SO.stem_case(B, H, W)
        r = {'x': put(x), 'bias': put(bias), 'k': put(k.reshape(147, 64)), 'absb': np.abs(bias.astype(np.float64))[None, None, None, :],
             'packed': hip.pack_stem_weights(k.reshape(147, 64), dev()), 'packed_x3': hip.pack_stem_weights_x3(k_dec.reshape(147, 64), dev()),
             'ref': SO.stem(x, k, bias), 'mag': SO.stem_abs(x, k),
             'ref_dec': SO.stem(x, k_dec, bias), 'mag_dec': SO.stem_abs(x, k_dec), 'pre_dec': SO.stem_sum(x, k_dec)}
        _REFS[key] = r
    return _REFS[key]


def guarded(shape, tdt):
    """ a NaN-poisoned output map with a guard row of its own behind it """
    n, guard = int(np.prod(shape)), int(shape[2] * shape[3])
    return torch.full((n + guard,), NAN, dtype=tdt, device=dev()), n


def collect(buf, n, shape):
    """ the map as float64; no NaN left inside it, the guard row untouched """
    host = buf.float().cpu().numpy() if buf.dtype != torch.float32 else buf.cpu().numpy()
    assert not np.isnan(host[:n]).any(), 'unwritten (or NaN) outputs: {}'.format(int(np.isnan(host[:n]).sum()))
    assert np.isnan(host[n:]).all(), 'wrote behind the map'
    return host[:n].reshape(shape).astype(np.float64)


def acc_term(r, mag, dt):
    return 149 * U * (mag + r['absb']) * (1.0 + U_OUT[dt])


def out_term(ref, dt):
    return U_OUT[dt] * np.abs(ref) + SUB_OUT[dt]


def assert_within(got, ref, tol, what):
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print('{}: worst err / tol {:.3f}, max err {:.3e}'.format(what, worst, float(err.max())))
    assert bool((err <= tol).all()), '{}: err / tol up to {:.3f} at {} of {} outputs'.format(what, worst, int((err > tol).sum()), err.size)


def x3_tolerance(r, Ho, Wo, B):
    """ elementwise: the magnitude bound everywhere, and on maps of >= 256 pixels the (tighter) project bar as well """
    ref, mag = r['ref_dec'], r['mag_dec']
    tol = 455 * U * mag + 1e-5 * np.abs(ref)
    rms_c = None
    if B * Ho * Wo >= 256:
        rms_c = np.sqrt((r['pre_dec'].reshape(-1, 64) ** 2).mean(axis=0))
        tol = np.minimum(tol, 1e-5 * np.abs(ref) + 2e-6 * 147 ** 0.5 * rms_c[None, None, None, :])
    return tol, rms_c


@pytest.mark.parametrize('dt', [hip.GPP_F32, hip.GPP_F16, hip.GPP_BF16], ids=['f32', 'f16', 'bf16'])
@pytest.mark.parametrize('B,H,W', SO.STEM_SHAPES)
def test_f32_stem_against_float64(B, H, W, dt):
    """ gpp_stem_conv7x7_bn_relu (stem_kernel: the fmaf chain on the vector ALUs), all three output types -- GPP_F32 is the reference
    path's stem and was compared with nothing.  TILE EDGES: Ho = 4 | 5 of the TH = 4 tile, Wo = 64 | 65 | 66 of the TW = 64 tile; PADDING:
    H, W < 7, where most of the 7 x 7 patch is the zero padding (1 x 1: 48 of 49 taps).  Bound: 149 u (mag + |b|) + output rounding. """
    r = stem_refs(B, H, W)
    Ho, Wo = conv_shape(H, W)
    out, n = guarded((B, Ho, Wo, 64), TDT[dt])
    hip.check(hip.lib().gpp_stem_conv7x7_bn_relu(hip.ptr(r['x']), hip.ptr(r['k']), hip.ptr(r['bias']), hip.ptr(out), dt, B, H, W, hip.stream_ptr()))
    got = collect(out, n, (B, Ho, Wo, 64))
    assert_within(got, r['ref'], acc_term(r, r['mag'], dt) + out_term(r['ref'], dt), 'f32 stem -> ' + NAMES[dt])


@pytest.mark.parametrize('dt', [hip.GPP_F16, hip.GPP_BF16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('B,H,W', SO.STEM_SHAPES)
def test_mfma_stem_and_its_fused_pool_against_float64(B, H, W, dt):
    """ gpp_stem_conv7x7_bn_relu_mfma (persistent 4-row x 64-column tiles, f16 operands) below 17 x 53 for the first time, and
    gpp_stem_pool_fused_mfma against maxpool_same(stem) -- an independent reference, not the unfused kernel.  TILE EDGES: Ho = 4 | 5,
    8 | 9 and Wo = 64 | 65 | 66; the fused form's strips of 31 pooled columns (Wp = 32, 33: a second strip of one or two columns) and
    row blocks of 4 pooled rows (Hp = 4, 5), its pre-step at pad_top = 0 (even Ho); PADDING: H, W < 7.
    Bound: 2^-10 mag + 149 u (mag + |b|) + output rounding; through the pool: a maximum moves by no more than the largest tolerance
    inside its window. """
    r = stem_refs(B, H, W)
    lib = hip.lib()
    Ho, Wo = conv_shape(H, W)
    tol = 2.0 ** -10 * r['mag'] + acc_term(r, r['mag'], dt) + out_term(r['ref'], dt)
    out, n = guarded((B, Ho, Wo, 64), TDT[dt])
    hip.check(lib.gpp_stem_conv7x7_bn_relu_mfma(hip.ptr(r['x']), hip.ptr(r['packed']), hip.ptr(r['bias']), hip.ptr(out), dt, B, H, W, hip.stream_ptr()))
    assert_within(collect(out, n, (B, Ho, Wo, 64)), r['ref'], tol, 'mfma stem -> ' + NAMES[dt])
    Hp, Wp = (Ho + 1) // 2, (Wo + 1) // 2
    pooled, n = guarded((B, Hp, Wp, 64), TDT[dt])
    hip.check(lib.gpp_stem_pool_fused_mfma(hip.ptr(r['x']), hip.ptr(r['packed']), hip.ptr(r['bias']), hip.ptr(pooled), dt, B, H, W, hip.stream_ptr()))
    assert_within(collect(pooled, n, (B, Hp, Wp, 64)), SO.maxpool_same(r['ref']), SO.maxpool_same(tol), 'fused mfma stem + pool -> ' + NAMES[dt])


@pytest.mark.parametrize('B,H,W', SO.STEM_SHAPES)
def test_x3_stem_and_its_fused_pool_against_float64(B, H, W):
    """ gpp_stem_conv7x7_bn_relu_x3 (persistent 8-row x 64-column tiles, hi / lo operands, weights four decades apart through the
    packer's per-channel scale) and gpp_stem_pool_fused_x3 (6 conv rows per step, the horizontal half of the pool in the accumulator
    lanes) against stem / maxpool_same(stem).  TILE EDGES: Ho = 8 | 9 of ROWS = 8, Wo = 64 | 65 | 66; fused: Hp = 3 | 4 of its 3 pooled
    rows per step, Wp = 32 | 33 of its 31-column strips, the DPP row shifts at a map narrower than one fragment; PADDING: H, W < 7.
    Bounds: see the module docstring (455 u mag + 1e-5 |ref| everywhere, the project's bars from 256 pixels on). """
    r = stem_refs(B, H, W)
    lib = hip.lib()
    Ho, Wo = conv_shape(H, W)
    tol, rms_c = x3_tolerance(r, Ho, Wo, B)
    out, n = guarded((B, Ho, Wo, 64), torch.float32)
    hip.check(lib.gpp_stem_conv7x7_bn_relu_x3(hip.ptr(r['x']), hip.ptr(r['packed_x3']), hip.ptr(r['bias']), hip.ptr(out), B, H, W, hip.stream_ptr()))
    got = collect(out, n, (B, Ho, Wo, 64))
    assert_within(got, r['ref_dec'], tol, 'x3 stem')
    if rms_c is not None:
        rms_err = np.sqrt(((got - r['ref_dec']).reshape(-1, 64) ** 2).mean(axis=0))
        print('x3 stem: rms(err) / rms_c up to {:.3e}'.format(float((rms_err / rms_c).max())))
        assert bool((rms_err <= 5e-7 * rms_c + 1e-8).all())
    Hp, Wp = (Ho + 1) // 2, (Wo + 1) // 2
    pooled, n = guarded((B, Hp, Wp, 64), torch.float32)
    slot = torch.zeros((1,), dtype=torch.int64, device=dev())
    hip.check(lib.gpp_stem_pool_fused_x3(hip.ptr(r['x']), hip.ptr(r['packed_x3']), hip.ptr(r['bias']), hip.ptr(pooled), B, H, W, slot.data_ptr(), hip.stream_ptr()))
    assert_within(collect(pooled, n, (B, Hp, Wp, 64)), SO.maxpool_same(r['ref_dec']), SO.maxpool_same(tol), 'fused x3 stem + pool')


# ----------------------------------------------------------------------------------------------------- 'same' max pool
FINFO_MAX = {hip.GPP_BF16: float(torch.finfo(torch.bfloat16).max), hip.GPP_F16: 65504.0, hip.GPP_F32: float(np.finfo(np.float32).max)}


def typed(values, dt):
    """ float32 values -> (device tensor of the type, the float32 array of what it holds) """
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(TDT[dt])
    return t.to(dev()).contiguous(), t.float().numpy()


@pytest.mark.parametrize('dt', [hip.GPP_BF16, hip.GPP_F16, hip.GPP_F32], ids=['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('H,W', [(1, 1), (1, 7), (2, 2), (3, 4), (19, 27), (20, 28)])
def test_maxpool_same_bit_exact(H, W, dt):
    """ gpp_maxpool3x3s2_same in all three types (GPP_F32 is what every x3 model runs; GPP_F16 had no independent reference) at
    C = 8, 24, 64 (one, three, eight vec8 items per pixel), B = 2, bit-exact.  PADDING VALUE: all-negative maps -- a zero padding would
    win every border window; 1 x 1, 1 x N and 2 x 2 maps, where every window is mostly padding; pad_total 2 (odd side: one before, one
    after) and 1 (even side: none before).  VALUES: +-inf and +- the largest finite number survive the float32 round trip. """
    rng = np.random.default_rng(H * 31 + W)
    for Cn in (8, 24, 64):
        neg = -(np.abs(rng.standard_normal((2, H, W, Cn))) + 0.01)
        big = FINFO_MAX[dt]
        ext = rng.choice(np.array([np.inf, -np.inf, big, -big, 1.5, -2.25, -1e-3], np.float64), size=(2, H, W, Cn))
        ext = np.where(rng.random((2, H, W, Cn)) < 0.5, ext, rng.standard_normal((2, H, W, Cn)))
        for name, values in (('negative', neg), ('extremes', ext)):
            xd, xh = typed(values, dt)
            assert name != 'negative' or bool((xh < 0).all())
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
            out, n = guarded((2, Ho, Wo, Cn), TDT[dt])
            hip.check(hip.lib().gpp_maxpool3x3s2_same(hip.ptr(xd), hip.ptr(out), dt, 2, H, W, Cn, hip.stream_ptr()))
            got = collect(out, n, (2, Ho, Wo, Cn))
            want = SO.maxpool_same(xh).astype(np.float64)
            assert np.array_equal(got, want), '{} C = {}: {} of {} differ'.format(name, Cn, int((got != want).sum()), got.size)


def test_maxpool_same_second_trip_of_the_stride_loop():
    """ STRIDE LOOP: the grid is capped at 8192 workgroups of 256 vec8 items; (1, 363, 363, 512) in f16 is the smallest square map of 512
    channels with more items than that (182 * 182 * 64 = 2 119 936 > 2 097 152), so the last 22 784 items are second trips.  Compared
    in chunks of 16 output rows; finite values of every magnitude and sign. """
    H = W = 363
    Cn = 512
    rng = np.random.default_rng(363)
    raw = rng.integers(0, 65536, size=(1, H, W, Cn), dtype=np.uint16)
    raw &= np.where((raw & 0x7C00) == 0x7C00, np.uint16(0xFBFF), np.uint16(0xFFFF))       # no inf / NaN: clear one exponent bit there
    x = raw.view(np.float16)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert Ho * Wo * (Cn // 8) > 8192 * 256 and (Ho - 1) * (Wo - 1) * (Cn // 8) <= 8192 * 256
    out, n = guarded((1, Ho, Wo, Cn), torch.float16)
    hip.check(hip.lib().gpp_maxpool3x3s2_same(hip.ptr(put(x)), hip.ptr(out), hip.GPP_F16, 1, H, W, Cn, hip.stream_ptr()))
    host = out.cpu().numpy()
    assert np.isnan(host[n:]).all()
    got = host[:n].reshape(1, Ho, Wo, Cn)
    x32 = x.astype(np.float32)                                # exact, and the maximum of floats is fast where that of halves is not
    for r0 in range(0, Ho, 16):
        r1 = min(r0 + 16, Ho)
        want = SO.maxpool_same(x32, rows=(r0, r1))
        assert np.array_equal(got[:, r0:r1].astype(np.float32), want), 'rows {} .. {}'.format(r0, r1)


def test_maxpool_same_error_codes():
    """ C % 8, a null pointer, a pointer off its 16 bytes, a type that is none of the three: -1, -1, -3, -4, and nothing is launched """
    lib = hip.lib()
    x = torch.zeros((1, 4, 4, 16), dtype=torch.float32, device=dev())
    out = torch.full((1, 2, 2, 16), 7.0, dtype=torch.float32, device=dev())
    st = hip.stream_ptr()
    assert lib.gpp_maxpool3x3s2_same(hip.ptr(x), hip.ptr(out), hip.GPP_F32, 1, 4, 4, 12, st) == -1
    assert lib.gpp_maxpool3x3s2_same(hip.ptr(x), hip.ptr(out), hip.GPP_F32, 1, 4, 4, 0, st) == -1
    assert lib.gpp_maxpool3x3s2_same(None, hip.ptr(out), hip.GPP_F32, 1, 4, 4, 16, st) == -1
    assert lib.gpp_maxpool3x3s2_same(hip.ptr(x), None, hip.GPP_F32, 1, 4, 4, 16, st) == -1
    assert lib.gpp_maxpool3x3s2_same(x.data_ptr() + 4, hip.ptr(out), hip.GPP_F32, 1, 4, 4, 8, st) == -3
    assert lib.gpp_maxpool3x3s2_same(hip.ptr(x), out.data_ptr() + 8, hip.GPP_F32, 1, 4, 4, 8, st) == -3
    assert lib.gpp_maxpool3x3s2_same(hip.ptr(x), hip.ptr(out), hip.GPP_F16X3, 1, 4, 4, 16, st) == -4
    assert lib.gpp_maxpool3x3s2_same(hip.ptr(x), hip.ptr(out), 0, 1, 4, 4, 16, st) == -4
    assert bool((out == 7.0).all())


# -------------------------------------------------------------------------------------------------- DenseNet's pools
def run_dense_pool(kind, x, pad, pitch):
    """ the pool into a NaN-poisoned buffer of `pitch` channels per pixel with a guard pixel behind it: (data, gap, guard) """
    B, H, W, Cn = x.shape
    Ho, Wo = ((H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1) if kind == 'max' else (H // 2, W // 2)
    buf = torch.full((B * Ho * Wo + 1, pitch), NAN, dtype=torch.float32, device=dev())
    xd = put(x)
    if kind == 'max':
        hip.check(hip.lib().gpp_maxpool3x3s2_pad_f32(hip.ptr(xd), hip.ptr(buf), B, H, W, Cn, pad, pitch, hip.stream_ptr()))
    else:
        hip.check(hip.lib().gpp_avgpool2x2_f32(hip.ptr(xd), hip.ptr(buf), B, H, W, Cn, pitch, hip.stream_ptr()))
    host = buf.cpu().numpy()
    return host[:-1, :Cn].reshape(B, Ho, Wo, Cn), host[:-1, Cn:], host[-1]


def assert_pool_bits(kind, x, pad, pitch):
    data, gap, guard = run_dense_pool(kind, x, pad, pitch)
    want = SO.maxpool_pad(x, pad) if kind == 'max' else SO.avgpool2x2(x)
    assert want.dtype == np.float32 and data.shape == want.shape
    assert np.array_equal(data.view(np.uint32), want.view(np.uint32)), '{} of {} differ'.format(int((data.view(np.uint32) != want.view(np.uint32)).sum()), want.size)
    assert np.isnan(gap).all() and np.isnan(guard).all(), 'wrote into the gap between pixels or behind the map'


@pytest.mark.parametrize('pad,H,W', [(1, 1, 1), (0, 3, 3), (1, 2, 5), (0, 33, 47), (1, 33, 47), (0, 32, 46), (1, 32, 46)])
def test_dense_maxpool_bit_exact(pad, H, W):
    """ gpp_maxpool3x3s2_pad_f32 on SIGNED inputs, bit-exact, B = 2.  PADDING VALUE: the kernel had only seen post-ReLU maps, where a
    zero padding and the documented -inf padding agree; on negative values they differ in every border window.  pad = 0 for the first
    time; the smallest legal maps (1 x 1 at pad 1: one window, eight of nine taps padding; 3 x 3 at pad 0); odd and even sizes (the last
    window ends on the map or on the padding).  C = 4 and 64 (one and sixteen vec4 items per pixel); out_pitch = C and C + 32: the 32
    channels between two pixels keep their sentinel. """
    rng = np.random.default_rng(100 * H + W + pad)
    for Cn in (4, 64):
        x = rng.standard_normal((2, H, W, Cn)).astype(np.float32)
        x[0] = -np.abs(x[0]) - 0.01                          # one image with nothing above zero at all
        for pitch in (Cn, Cn + 32):
            assert_pool_bits('max', x, pad, pitch)


@pytest.mark.parametrize('H,W', [(2, 2), (3, 2), (2, 3), (33, 47), (32, 46)])
def test_dense_avgpool_bit_exact(H, W):
    """ gpp_avgpool2x2_f32 on signed inputs, bit-exact against ((x00 + x01) + x10) + x11 then * 0.25 in float32, B = 2.  FLOOR: an odd
    last row / column (33 x 47, 3 x 2, 2 x 3) is dropped and never read into a window; the smallest legal map 2 x 2; C = 4 and 64;
    out_pitch = C and C + 32 with the gap's sentinel intact.  Cancelling signed terms make the order of the sum visible. """
    rng = np.random.default_rng(100 * H + W)
    for Cn in (4, 64):
        x = (rng.standard_normal((2, H, W, Cn)) * np.power(10.0, rng.integers(-3, 4, size=(2, H, W, Cn)))).astype(np.float32)
        for pitch in (Cn, Cn + 32):
            assert_pool_bits('avg', x, 0, pitch)


@pytest.fixture(scope='module')
def big_signed_map():
    """ (1, 726, 726, 64) float32, shared by the two stride-loop cases of dense_pool_kernel and dropped with the module """
    return np.random.default_rng(726).standard_normal((1, 726, 726, 64), dtype=np.float32)


def test_dense_maxpool_second_trip_of_the_stride_loop(big_signed_map):
    """ STRIDE LOOP of dense_pool_kernel<false>: 8192 x 256 vec4 items; (1, 725, 725, 64) at pad 1 gives 363 * 363 * 16 = 2 108 304 items
    (362 * 362 * 16 fits), so the last 11 152 are second trips """
    x = np.ascontiguousarray(big_signed_map[:, :725, :725])
    assert 363 * 363 * 16 > 8192 * 256 >= 362 * 362 * 16
    assert_pool_bits('max', x, 1, 64)


def test_dense_avgpool_second_trip_of_the_stride_loop(big_signed_map):
    """ STRIDE LOOP of dense_pool_kernel<true>: (1, 726, 726, 64) -> 363 x 363 x 16 vec4 items, 11 152 of them second trips """
    assert_pool_bits('avg', big_signed_map, 0, 64)


def test_dense_pool_error_codes():
    """ what check_args and the two entry points promise: -1 for C % 4, out_pitch < C, out_pitch % 4, null pointers, a map smaller than
    one window (H + 2 pad < 3; H < 2 for the average); -3 for a pointer off its 16 bytes; -4 for pad outside {0, 1} and for a map of
    2^40 elements; nothing is launched """
    lib = hip.lib()
    x = torch.zeros((1, 4, 4, 8), dtype=torch.float32, device=dev())
    out = torch.full((64,), 7.0, dtype=torch.float32, device=dev())
    st = hip.stream_ptr()
    px, po = hip.ptr(x), hip.ptr(out)
    mx, av = lib.gpp_maxpool3x3s2_pad_f32, lib.gpp_avgpool2x2_f32
    assert mx(px, po, 1, 4, 4, 6, 1, 8, st) == -1 and av(px, po, 1, 4, 4, 6, 8, st) == -1            # C % 4
    assert mx(px, po, 1, 4, 4, 8, 1, 4, st) == -1 and av(px, po, 1, 4, 4, 8, 4, st) == -1            # out_pitch < C
    assert mx(px, po, 1, 4, 4, 8, 1, 10, st) == -1 and av(px, po, 1, 4, 4, 8, 10, st) == -1          # out_pitch % 4
    assert mx(None, po, 1, 4, 4, 8, 1, 8, st) == -1 and av(px, None, 1, 4, 4, 8, 8, st) == -1
    assert mx(px, po, 0, 4, 4, 8, 1, 8, st) == -1 and av(px, po, 1, 0, 4, 8, 8, st) == -1
    assert mx(px, po, 1, 2, 4, 8, 0, 8, st) == -1 and mx(px, po, 1, 4, 2, 8, 0, 8, st) == -1         # H + 2 pad < 3, W + 2 pad < 3
    assert mx(px, po, 1, 1, 1, 8, 0, 8, st) == -1 and mx(px, po, 1, 1, 1, 8, 1, 8, st) == 0          # (1 x 1 is legal at pad 1)
    assert av(px, po, 1, 1, 4, 8, 8, st) == -1 and av(px, po, 1, 4, 1, 8, 8, st) == -1               # H < 2, W < 2
    assert mx(x.data_ptr() + 4, po, 1, 4, 4, 8, 1, 8, st) == -3 and av(px, out.data_ptr() + 8, 1, 4, 4, 8, 8, st) == -3
    assert mx(px, po, 1, 4, 4, 8, 2, 8, st) == -4 and mx(px, po, 1, 4, 4, 8, -1, 8, st) == -4
    assert mx(px, po, 1 << 15, 1 << 15, 1 << 10, 4, 1, 4, st) == -4 and av(px, po, 1 << 15, 1 << 15, 1 << 10, 4, 4, st) == -4
    torch.cuda.synchronize()
    assert bool((out[8:] == 7.0).all())                       # (the one legal call wrote the first pixel)


# ----------------------------------------------------------------------------------------------------------------- ReLU
RAW = {hip.GPP_BF16: (torch.int16, np.uint16, 16), hip.GPP_F16: (torch.int16, np.uint16, 16), hip.GPP_F32: (torch.int32, np.uint32, 32),
       hip.GPP_BF16X3: (torch.int16, np.uint16, 16), hip.GPP_F16X3: (torch.int16, np.uint16, 16)}
# +-0, +-inf, +- largest finite, +- smallest subnormal, +-1
SPECIALS = {hip.GPP_F16: [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x3C00, 0xBC00, 0x03FF, 0x83FF],
            hip.GPP_BF16: [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x3F80, 0xBF80, 0x007F, 0x807F],
            hip.GPP_F32: [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000,
                          0x007FFFFF, 0x807FFFFF]}
# (hi, lo) of a pre-split pair: negative f16 subnormals whose bits are bf16 subnormals too (0x8001 .. 0x807F: the kernel reads both x3 types as
# bf16 and compares a float32 SUBNORMAL with zero), the first word that is a normal bf16 (0x8080), the last f16 subnormal (0x83FF); -0.0 with a
# zero, a positive and a negative lo; hi > 0 with lo < 0; hi < 0 with lo > 0; the smallest positive hi
X3_PAIRS = [(0x8001, 0x0155), (0x8040, 0x8155), (0x807F, 0x0001), (0x8080, 0x0155), (0x83FF, 0x8001), (0x8001, 0x0000),
            (0x8000, 0x0000), (0x8000, 0x0001), (0x8000, 0x8001), (0x3C00, 0x9000), (0x0400, 0x8001), (0xBC00, 0x1000), (0xFBFF, 0x7BFF),
            (0x0001, 0x8155), (0x0000, 0x8001), (0x7BFF, 0xFBFF)]


def relu_strided(inp, ibs, out, obs, dt, B, count):
    """ (the one entry point hip.py declares no argument types for: the 64-bit ones are passed as such) """
    return hip.lib().gpp_relu_strided(ctypes.c_void_p(inp), ctypes.c_int64(ibs), ctypes.c_void_p(out), ctypes.c_int64(obs), ctypes.c_int(dt),
                                      ctypes.c_int(B), ctypes.c_int64(count), hip.stream_ptr())


def finite_words(rng, n, npdt, dt):
    """ random words of every magnitude and sign (subnormals included) that are no inf / NaN of the type """
    if npdt == np.uint32:
        w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        return np.where((w & 0x7F800000) == 0x7F800000, w & np.uint32(0xBFFFFFFF), w)
    w = rng.integers(0, 65536, size=n, dtype=np.uint16)
    expo = np.uint16(0x7F80 if dt == hip.GPP_BF16 else 0x7C00)
    return np.where((w & expo) == expo, w & np.uint16(0xBFFF), w)


def x3_image(rng, dt, groups):
    """ groups x [32 hi | 32 lo] raw words: the hand-written pairs first, then ordinary values split by FMap.write """
    fm = C.FMap.empty(1, 1, groups, 32, torch.float32, dev(), split=True, half=NAMES[dt])
    fm.write(torch.from_numpy(rng.standard_normal((1, 1, groups, 32)).astype(np.float32) * 3.0))
    words = fm.buf.view(torch.int16).cpu().numpy().view(np.uint16).reshape(groups, 2, 32).copy()
    for i, (h, l) in enumerate(X3_PAIRS):
        words[0, 0, i], words[0, 1, i] = h, l
    return words


def relu_expected(words, dt):
    """ (expected words, mask of the inputs for which either zero is right: -0.0 under the plain kernels) """
    _, npdt, bits = RAW[dt]
    if dt in (hip.GPP_BF16X3, hip.GPP_F16X3):
        w = words.reshape(-1, 2, 32)
        hi, lo = SO.relu_split_halves(w[:, 0], w[:, 1])
        return np.stack([hi, lo], axis=1).reshape(words.shape), np.zeros(words.shape, bool)
    return SO.relu_words(words, bits), words == npdt(1 << (bits - 1))


def assert_relu_words(got, want, either, bits, what):
    sign = got.dtype.type(1 << (bits - 1))
    ok = np.where(either, (got & ~sign) == 0, got == want)
    assert bool(ok.all()), '{}: {} of {} words differ, first at {}: got {:#x}, want {:#x}'.format(
        what, int((~ok).sum()), ok.size, int(np.flatnonzero(~ok)[0]), int(got.reshape(-1)[np.flatnonzero(~ok)[0]]), int(want.reshape(-1)[np.flatnonzero(~ok)[0]]))


@pytest.mark.parametrize('dt', [hip.GPP_BF16, hip.GPP_F16, hip.GPP_F32, hip.GPP_BF16X3, hip.GPP_F16X3], ids=['bf16', 'f16', 'f32', 'bf16x3', 'f16x3'])
def test_relu_strided_raw_words(dt):
    """ gpp_relu_strided (called from no test before) on raw words, B = 3, in_bstride = count + 32 != out_bstride = count + 96: every
    image is read and written at its own stride, the elements between two images keep their sentinel (input AND output side), and
    GPP_F16 runs for the first time.  HALF-WORD PATTERNS, plain types: +-0, +-inf, +- largest finite, +- smallest and largest subnormal
    (a flushed subnormal would show as a changed word), +-1, random finite words.  x3 types: the pairs of X3_PAIRS -- a negative f16
    subnormal hi is a float32 subnormal in relu_x3_kernel's comparison and must still clear the pair; hi = -0.0 and hi > 0 with a
    negative lo must not.  The same words through gpp_relu (B = 1, strides 0) for the first image. """
    tdt, npdt, bits = RAW[dt]
    x3 = dt in (hip.GPP_BF16X3, hip.GPP_F16X3)
    per = 4 // (bits // 8) if x3 else 1                       # words per counted element: x3 maps are counted in float32-sized elements
    count = 288
    B, ibs, obs = 3, count + 32, count + 96
    rng = np.random.default_rng(dt)
    images = []
    for b in range(B):
        if x3:
            images.append(x3_image(rng, dt, count // 32).reshape(-1))
        else:
            sp = np.array(SPECIALS[dt], npdt)
            images.append(np.concatenate([sp, finite_words(rng, count - sp.size, npdt, dt)]))
    sent_in, sent_out = npdt(0x5A5A), npdt(0x3A3A)
    src = np.full((B * ibs * per,), sent_in, npdt)
    for b in range(B):
        src[b * ibs * per:b * ibs * per + count * per] = images[b]
    sd = put(src.view({np.uint16: np.int16, np.uint32: np.int32}[npdt]))
    od = torch.full((B * obs * per,), int(sent_out), dtype=tdt, device=dev())
    assert relu_strided(sd.data_ptr(), ibs, od.data_ptr(), obs, dt, B, count) == 0
    got = od.cpu().numpy().view(npdt)
    assert np.array_equal(sd.cpu().numpy().view(npdt), src)                       # the input is read only
    for b in range(B):
        want, either = relu_expected(images[b], dt)
        assert_relu_words(got[b * obs * per:b * obs * per + count * per], want, either, bits, 'image {}'.format(b))
        assert bool((got[b * obs * per + count * per:(b + 1) * obs * per] == sent_out).all()), 'gap behind image {} written'.format(b)
    one = torch.full((count * per + 64,), int(sent_out), dtype=tdt, device=dev())
    assert hip.lib().gpp_relu(hip.ptr(sd), hip.ptr(one), dt, count, hip.stream_ptr()) == 0
    got = one.cpu().numpy().view(npdt)
    want, either = relu_expected(images[0], dt)
    assert_relu_words(got[:count * per], want, either, bits, 'gpp_relu')
    assert bool((got[count * per:] == sent_out).all())


@pytest.mark.parametrize('dt', [hip.GPP_F16, hip.GPP_F16X3], ids=['f16', 'f16x3'])
def test_relu_second_trip_of_the_stride_loop(dt):
    """ STRIDE LOOP of relu_kernel and relu_x3_kernel: 4096 x 256 vec8 items per image; count = 8 388 608 + 32 is the smallest count
    (a multiple of 32) with more, so the last four items are second trips.  Random finite words, through gpp_relu. """
    tdt, npdt, bits = RAW[dt]
    x3 = dt == hip.GPP_F16X3
    per = 2 if x3 else 1
    count = 4096 * 256 * 8 + 32
    assert count // 8 > 4096 * 256 >= (count - 32) // 8
    rng = np.random.default_rng(4096 + dt)
    words = finite_words(rng, count * per, npdt, hip.GPP_F16)
    sd = put(words.view(np.int16))
    od = torch.full((count * per + 64,), 0x3A3A, dtype=tdt, device=dev())
    assert hip.lib().gpp_relu(hip.ptr(sd), hip.ptr(od), dt, count, hip.stream_ptr()) == 0
    got = od.cpu().numpy().view(npdt)
    want, either = relu_expected(words, dt)
    assert_relu_words(got[:count * per], want, either, bits, 'gpp_relu, {} elements'.format(count))
    assert bool((got[count * per:] == 0x3A3A).all())


def test_relu_error_codes():
    """ count % 8 (x3: count % 32), a batch stride that is no multiple of 8 (x3: of 32), null and misaligned pointers, B = 0, a type
    that is none of the five: -1, -1, -1, -3, -1, -4; nothing is launched """
    x = torch.zeros((256,), dtype=torch.float32, device=dev())
    out = torch.full((256,), 7.0, dtype=torch.float32, device=dev())
    a, o = x.data_ptr(), out.data_ptr()
    assert relu_strided(a, 64, o, 64, hip.GPP_F32, 2, 60) == -1
    assert relu_strided(a, 64, o, 64, hip.GPP_F32, 2, 0) == -1
    assert relu_strided(a, 64, o, 64, hip.GPP_F16X3, 2, 40) == -1 and relu_strided(a, 64, o, 64, hip.GPP_BF16X3, 2, 56) == -1
    assert relu_strided(a, 68, o, 64, hip.GPP_F32, 2, 64) == -1 and relu_strided(a, 64, o, 68, hip.GPP_F32, 2, 64) == -1
    assert relu_strided(a, 72, o, 64, hip.GPP_F16X3, 2, 64) == -1 and relu_strided(a, 64, o, 72, hip.GPP_BF16X3, 2, 64) == -1
    assert relu_strided(0, 64, o, 64, hip.GPP_F32, 2, 64) == -1 and relu_strided(a, 64, 0, 64, hip.GPP_F32, 2, 64) == -1
    assert relu_strided(a, 64, o, 64, hip.GPP_F32, 0, 64) == -1
    assert relu_strided(a + 4, 64, o, 64, hip.GPP_F32, 2, 64) == -3 and relu_strided(a, 64, o + 8, 64, hip.GPP_F16X3, 2, 64) == -3
    assert relu_strided(a, 64, o, 64, 0, 2, 64) == -4 and relu_strided(a, 64, o, 64, 6, 2, 64) == -4
    assert hip.lib().gpp_relu(hip.ptr(x), hip.ptr(out), hip.GPP_F32, 12, hip.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
