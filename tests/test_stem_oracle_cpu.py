"""
The float64 oracle of the stem / pooling / ReLU family (tests/stem_oracle.py) against torch's float64 conv2d and max_pool2d -- so that
the oracle is itself checked by code it shares nothing with --, the two host-side stem weight packers (device-free: they run here)
against the oracle's restatement of the packed layouts, byte for byte, and the operand parts of the error bounds that
tests/test_stem_edges_gpu.py asserts on the kernels, shown on the CPU on that file's inputs with no kernel involved.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_oracle as SO
from keras_retinanet_3D.backend import hip

F16_BYTES = 64 * 232 * 2
X3_BYTES = 2 * F16_BYTES + 64 * 4


# ------------------------------------------------------------------------------------------------- the oracle is honest
@pytest.mark.parametrize('B,H,W', [(1, 1, 1), (1, 2, 3), (2, 7, 9), (1, 16, 21), (2, 13, 18)])
def test_stem_oracle_matches_torch_float64(B, H, W):
    """ zero pad 3, 7x7 stride 2, bias, ReLU -- and sum |x||w| -- against F.conv2d in float64: patches that are mostly padding, odd and
    even sizes, more than one image """
    x, k, _, bias = SO.stem_case(B, H, W)
    xt, kt = torch.from_numpy(x.copy()).double().permute(0, 3, 1, 2), torch.from_numpy(k.copy()).double().permute(3, 2, 0, 1)
    want = torch.relu(F.conv2d(F.pad(xt, (3, 3, 3, 3)), kt, torch.from_numpy(bias.copy()).double(), stride=2)).permute(0, 2, 3, 1).numpy()
    want_abs = F.conv2d(F.pad(xt.abs(), (3, 3, 3, 3)), kt.abs(), None, stride=2).permute(0, 2, 3, 1).numpy()
    got, got_abs = SO.stem(x, k, bias), SO.stem_abs(x, k)
    assert got.shape == want.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64) and got.dtype == np.float64
    assert np.all(np.abs(got - want) <= 1e-12 * want_abs + 1e-300)
    assert np.all(np.abs(got_abs - want_abs) <= 1e-12 * want_abs)


@pytest.mark.parametrize('H,W', [(1, 1), (1, 7), (2, 2), (3, 4), (19, 27), (20, 28)])
def test_pool_oracles_match_torch(H, W):
    """ TF 'same' (pad_before = pad_total // 2) and the explicit symmetric padding, -inf in both, against F.max_pool2d on signed
    float64 values; the average pool against F.avg_pool2d and against its own definition written as a loop """
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((2, H, W, 8))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pt, pl = max((Ho - 1) * 2 + 3 - H, 0), max((Wo - 1) * 2 + 3 - W, 0)
    want = F.max_pool2d(F.pad(xt, (pl // 2, pl - pl // 2, pt // 2, pt - pt // 2), value=float('-inf')), 3, 2).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(SO.maxpool_same(x), want)
    for r0, r1 in ((0, 1), (0, Ho), (Ho - 1, Ho), (Ho // 2, Ho)):                       # the chunked form a large map is compared with
        assert np.array_equal(SO.maxpool_same(x, rows=(r0, r1)), want[:, r0:r1])
    for pad in (0, 1):
        if H + 2 * pad < 3 or W + 2 * pad < 3:
            continue
        want = F.max_pool2d(F.pad(xt, (pad, pad, pad, pad), value=float('-inf')), 3, 2).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(SO.maxpool_pad(x, pad), want)
    if H >= 2 and W >= 2:
        x32 = x.astype(np.float32)
        got = SO.avgpool2x2(x32)
        assert got.dtype == np.float32 and got.shape == (2, H // 2, W // 2, 8)
        want = F.avg_pool2d(torch.from_numpy(x32).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy()
        assert np.allclose(got, want, rtol=1e-6, atol=1e-7)
        for y in range(H // 2):
            for xx in range(W // 2):
                a, b, c, d = x32[:, 2 * y, 2 * xx], x32[:, 2 * y, 2 * xx + 1], x32[:, 2 * y + 1, 2 * xx], x32[:, 2 * y + 1, 2 * xx + 1]
                assert np.array_equal(got[:, y, xx], np.float32(np.float32(np.float32(a + b) + c) + d) * np.float32(0.25))


def test_relu_oracles_on_hand_written_words():
    """ negative non-zero -> +0 (subnormals and -inf too), everything else -- -0.0, +subnormal, +inf -- unchanged; a pair follows its hi """
    words = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF, 0x3C00, 0xBC00], np.uint16)
    assert SO.relu_words(words, 16).tolist() == [0x0000, 0x8000, 0x0001, 0, 0x7C00, 0, 0x7BFF, 0, 0x3C00, 0]
    assert SO.relu_words(np.array([0x80000001, 0x00000001, 0xFF800000, 0x80000000], np.uint32), 32).tolist() == [0, 1, 0, 0x80000000]
    hi = np.array([0x8001, 0x8000, 0x3C00, 0xBC00, 0x0000], np.uint16)
    lo = np.array([0x0123, 0x0456, 0x8789, 0x0789, 0x8001], np.uint16)
    h, l = SO.relu_split_halves(hi, lo)
    assert h.tolist() == [0, 0x8000, 0x3C00, 0, 0x0000] and l.tolist() == [0, 0x0456, 0x8789, 0, 0x8001]


# ------------------------------------------------------------------------------------------------------- the packers
def _unit_channel(rng):
    """ 147 weights with largest magnitude exactly 1, the rest spread down to 1e-4 of it """
    v = rng.standard_normal(147) * np.power(10.0, rng.uniform(-4.0, 0.0, 147))
    v /= np.abs(v).max()
    return v


def _weights(case):
    """ (147, 64) float32 and the channels the case is about; every case starts from the ordinary draw """
    rng = np.random.default_rng(7)
    w = (rng.standard_normal((147, 64)) * 0.05).astype(np.float32)
    chans = {
        'ordinary': {},
        'zero_channel': {5: 0.0, 40: 0.0},
        'nine_decades': {2: 1e-5, 3: 1e4, 34: 3e-3, 61: 2.5},
        'amax_3e38': {17: 3e38},
        'amax_1e-30': {9: 1e-30},
        'amax_4.9e-35': {22: 4.9e-35},             # just above 2^-114 = 4.81e-35: the unbounded exponent is 127, out_scale subnormal
        'amax_4.7e-35': {22: 4.7e-35, 63: 4.7e-35},  # just below: the unbounded exponent is 128, 2^128 = inf
        'amax_1e-36': {0: 1e-36, 31: 1e-36},
        'subnormal': {12: 1e-40, 45: 7e-45, 50: 2.4e-38},   # float32 subnormals (7e-45 = 5 quanta), and a channel straddling 2^-126
    }[case]
    for n, amax in chans.items():
        w[:, n] = (_unit_channel(rng) * amax).astype(np.float32)
    return w, sorted(chans)


PACK_CASES = ['ordinary', 'zero_channel', 'nine_decades', 'amax_3e38', 'amax_1e-30', 'amax_4.9e-35', 'amax_4.7e-35', 'amax_1e-36', 'subnormal']


def _pack_x3(w):
    dst = np.full((X3_BYTES + 64,), 0xA5, np.uint8)
    rc = hip.lib().gpp_stem_pack_weights_f16x3(w.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p), X3_BYTES)
    assert rc == 0 and bool((dst[X3_BYTES:] == 0xA5).all())          # nothing written past the blob
    blob = dst[:X3_BYTES]
    hi = blob[:F16_BYTES].view(np.float16).reshape(64, 232)
    lo = blob[F16_BYTES:2 * F16_BYTES].view(np.float16).reshape(64, 232)
    return blob, hi, lo, blob[2 * F16_BYTES:].view(np.float32)


def _pack_f16(w):
    dst = np.full((F16_BYTES + 64,), 0xA5, np.uint8)
    rc = hip.lib().gpp_stem_pack_weights_f16(w.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p), F16_BYTES)
    assert rc == 0 and bool((dst[F16_BYTES:] == 0xA5).all())
    return dst[:F16_BYTES]


def _pad_slots():
    k = np.arange(232)
    return (k >= 224) | (k % 32 >= 21)


@pytest.mark.parametrize('case', PACK_CASES)
def test_f16_packer_bytes_equal_the_oracle(case):
    """ gpp_stem_pack_weights_f16: row interleave (row 16h + 4q + r = channel 8q + 4h + r), k = kh * 32 + kw * 3 + c, pitch 232, round to
    nearest even, the 85 unused slots of every row exactly +0 -- byte for byte (a plain cast: 3e38 packs as inf here, by definition) """
    w, _ = _weights(case)
    got = _pack_f16(w)
    assert got.tobytes() == SO.pack_f16(w).tobytes()
    assert bool((got.view(np.uint16).reshape(64, 232)[:, _pad_slots()] == 0).all())


@pytest.mark.parametrize('case', PACK_CASES)
def test_x3_packer_bytes_equal_the_oracle(case):
    """ gpp_stem_pack_weights_f16x3: the layout of the f16 packer twice (hi, lo) + out_scale by channel, the scale 2^e that brings amax
    into [2^13, 2^14) with e bounded to +-126 -- byte for byte.  'ordinary' pins that the bound changed nothing inside the working
    range; the tiny channels are the ones whose unbounded exponent (127 .. 162) gave out_scale subnormal / zero and 2^e = inf """
    w, _ = _weights(case)
    blob, _, _, _ = _pack_x3(w)
    assert blob.tobytes() == SO.pack_f16x3_bytes(w)


@pytest.mark.parametrize('case', PACK_CASES)
def test_x3_packed_channels_are_finite_and_reproduce_the_weights(case):
    """ what the kernel will multiply with, for EVERY channel of every case: hi, lo and out_scale finite, out_scale a normal power of two
    (the exact inverse of the scale), the padded k slots exactly +0 in both halves, and (hi + lo) * out_scale == w
      * to 2^-21 of the channel's amax where the scaled weight is a normal half (hi and lo keep 11 bits each: 2^-22 |v| from a normal
        lo, 2^-25 absolute from a subnormal one, and amax 2^e >= 2^-4 whenever a rounding happens at all),
      * to one ulp of a subnormal half, 2^-24 * out_scale, where the scaled weight is below 2^-14.
    Before the exponent was bounded this failed for amax < 2^-114: hi = +-inf, lo and the padded slots NaN, out_scale 2^-128 (subnormal)
    or 0; and at amax in [2^-114, 2^-113) out_scale was the subnormal 2^-127. """
    w, _ = _weights(case)
    _, hi, lo, out_scale = _pack_x3(w)
    assert np.isfinite(hi.astype(np.float64)).all() and np.isfinite(lo.astype(np.float64)).all(), \
        'channels with non-finite halves: {}'.format(sorted(set(SO.packed_rows()[np.nonzero(~np.isfinite(hi.astype(np.float64) + lo.astype(np.float64)))[0]].tolist())))
    assert np.isfinite(out_scale).all() and bool((out_scale >= np.float32(2.0 ** -126)).all()), out_scale
    mant, _ = np.frexp(out_scale.astype(np.float64))
    assert bool((mant == 0.5).all())                                                    # powers of two
    pad = _pad_slots()
    assert bool((hi.view(np.uint16)[:, pad] == 0).all()) and bool((lo.view(np.uint16)[:, pad] == 0).all())
    rows = SO.packed_rows()
    for pos in range(64):
        n = int(rows[pos])
        s = np.float64(out_scale[n])
        rec = np.concatenate([(hi[pos].astype(np.float64) + lo[pos].astype(np.float64))[kh * 32:kh * 32 + 21] for kh in range(7)]) * s
        wn = w[:, n].astype(np.float64)
        amax = np.abs(wn).max()
        scaled = np.abs(wn) / s
        assert scaled.max() < 2.0 ** 14 and (amax == 0 or scaled.max() >= 2.0 ** 13 or s == 2.0 ** -126), (n, scaled.max())
        tol = np.where(scaled >= 2.0 ** -14, 2.0 ** -21 * amax, 2.0 ** -24 * s)
        err = np.abs(rec - wn)
        assert bool((err <= tol).all()), 'channel {}: amax {:g}, out_scale {:g}, worst err / tol {:g}'.format(n, amax, s, (err / tol).max())


def test_packers_refuse_small_buffers_and_null_pointers():
    lib = hip.lib()
    w, _ = _weights('ordinary')
    dst = np.zeros((X3_BYTES,), np.uint8)
    src, out = w.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p)
    assert lib.gpp_stem_pack_weights_f16(src, out, F16_BYTES - 1) == -1
    assert lib.gpp_stem_pack_weights_f16(None, out, F16_BYTES) == -1
    assert lib.gpp_stem_pack_weights_f16(src, None, F16_BYTES) == -1
    assert lib.gpp_stem_pack_weights_f16x3(src, out, X3_BYTES - 1) == -1
    assert lib.gpp_stem_pack_weights_f16x3(src, out, 2 * F16_BYTES) == -1              # the halves fit, out_scale does not
    assert lib.gpp_stem_pack_weights_f16x3(None, out, X3_BYTES) == -1
    assert lib.gpp_stem_pack_weights_f16x3(src, None, X3_BYTES) == -1
    assert not dst.any()                                                               # a refused call writes nothing


# ------------------------------------------------------------- the operand parts of the GPU bounds, with no kernel involved
@pytest.mark.parametrize('B,H,W', SO.STEM_SHAPES)
def test_rounded_operands_stay_inside_the_operand_terms_of_the_gpu_bounds(B, H, W):
    """ tests/test_stem_edges_gpu.py bounds a kernel's error by (operand term) + (float32 accumulation term).  The operand terms are
    derived from the number formats; here the float64 evaluation of the ROUNDED operands is shown to stay inside them on that file's
    inputs, so that what is left to the kernel is its float32 accumulation alone:
      * MFMA stem: x and w rounded to f16, 2^-11 relative each -> 2^-10 sum |x||w| (second order 2^-22, subnormal halves: absorbed by
        the fact that the roundings do not all point the same way -- shown here, not assumed);
      * x3 stem: each operand keeps hi + lo (2^-22 relative), the lo * lo product (<= 2^-22 |x||w|) is dropped -> 3 * 2^-22 sum |x||w|,
        on the weights the packer (and the oracle's restatement of it) scales per channel. """
    x, k, k_decades, bias = SO.stem_case(B, H, W)
    b64 = bias.astype(np.float64)[None, None, None, :]
    ref, mag = SO.stem(x, k, bias), SO.stem_abs(x, k)
    model = np.maximum(SO.stem_sum(x.astype(np.float16).astype(np.float64), k.astype(np.float16).astype(np.float64)) + b64, 0.0)
    assert bool((np.abs(model - ref) <= 2.0 ** -10 * mag).all()), (np.abs(model - ref) / mag).max()

    ref, mag = SO.stem(x, k_decades, bias), SO.stem_abs(x, k_decades)
    xh, xl = SO.split_f16(x)
    e = np.array([SO.x3_exponent(np.abs(k_decades[..., n]).max()) for n in range(64)])
    wh, wl = SO.split_f16(k_decades * np.ldexp(1.0, e).astype(np.float32)[None, None, None, :])
    acc = SO.stem_sum(xh + xl, wh + wl) - SO.stem_sum(xl, wl)                       # hi*hi + hi*lo + lo*hi
    model = np.maximum(acc * np.ldexp(1.0, -e)[None, None, None, :] + b64, 0.0)
    assert bool((np.abs(model - ref) <= 3 * 2.0 ** -22 * mag).all()), (np.abs(model - ref) / mag).max()
