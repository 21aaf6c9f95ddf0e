"""
Float64 oracle of the stem / pooling / ReLU family (csrc/stem.hip, csrc/stem_kernels.h, csrc/densenet.hip): plain NumPy, written from the
layer definitions and from the layout comments of include/gpp.h -- no torch operation, no project code.  The tests compare the HIP kernels
and the host-side weight packers with these functions; tests/test_stem_oracle_cpu.py compares these functions with torch's float64 conv2d
and max_pool2d, so that the oracle itself is checked by something it does not share a line with.

Maps are NHWC arrays.  Maxima are exact (they return one of their inputs), so the pooling functions keep the dtype they are given.
"""
import numpy as np

STEM_PITCH = 232                 # halfs per packed weight row: 7 kernel rows x 32 slots (21 used), + 8
X3_EXP_MIN, X3_EXP_MAX = -126, 126     # 2^e and 2^-e are both NORMAL float32 numbers for every e in this range


# --------------------------------------------------------------------------------------------------------------- stem
def stem_sum(x, k):
    """ ZeroPadding2D(3) + Conv2D(64, 7x7, stride 2, 'valid', no bias) in float64: x (B, H, W, 3), k (7, 7, 3, 64) -> (B, Ho, Wo, 64) """
    x = np.asarray(x, np.float64)
    k = np.asarray(k, np.float64)
    B, H, W, _ = x.shape
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    xp = np.zeros((B, H + 6, W + 6, 3), np.float64)
    xp[:, 3:3 + H, 3:3 + W] = x
    out = np.zeros((B, Ho, Wo, k.shape[3]), np.float64)
    for kh in range(7):
        for kw in range(7):
            out += xp[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2, :] @ k[kh, kw]
    return out


def stem(x, k, bias):
    """ conv1 + folded BatchNormalization + ReLU: max(conv(x, k) + bias, 0) """
    return np.maximum(stem_sum(x, k) + np.asarray(bias, np.float64)[None, None, None, :], 0.0)


def stem_abs(x, k):
    """ sum |x| |w| over the taps of every output: what the error bounds of the kernels are proportional to """
    return stem_sum(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(k, np.float64)))


def split_f16(a):
    """ the two IEEE halves the x3 kernels keep of a float32 operand: hi = f16(a), lo = f16(a - hi), as float64 values """
    a = np.asarray(a, np.float32)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


# the shapes (B, H, W) of tests/test_stem_edges_gpu.py: patches that are mostly padding (H or W below 7), and conv maps of exactly one
# tile and one more -- Ho = 4 | 5 (TH = 4), Ho = 8 | 9 (ROWS = 8), Wo = 64 | 65 | 66 (TW = 64)
STEM_SHAPES = [(1, 1, 1), (1, 2, 3), (1, 6, 6), (2, 7, 9), (1, 8, 127), (1, 9, 129), (1, 16, 130), (3, 17, 131)]
_CASES = {}


def stem_case(B, H, W):
    """ the seeded inputs of one shape, float32: mean-subtracted pixels x, a folded kernel k (7, 7, 3, 64), the same kernel with its
    channels spread over four decades (k_decades: the per-channel scale of the x3 packer at work) and a bias.  Computed once. """
    key = (B, H, W)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * H + W + B)
        x = (rng.random((B, H, W, 3), dtype=np.float32) * np.float32(255.0) - np.float32(120.0)).astype(np.float32)
        k = (rng.standard_normal((7, 7, 3, 64)) * 0.05).astype(np.float32)
        k_decades = (k * np.power(10.0, np.linspace(-2.0, 2.0, 64))[None, None, None, :]).astype(np.float32)
        bias = rng.standard_normal(64).astype(np.float32)
        for a in (x, k, k_decades, bias):
            a.setflags(write=False)
        _CASES[key] = (x, k, k_decades, bias)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------ pooling
def _window_max(xp, Ho, Wo):
    out = None
    for dy in range(3):
        for dx in range(3):
            v = xp[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2, :]
            out = v.copy() if out is None else np.maximum(out, v)
    return out


def _padded(x, top, bottom, left, right, value):
    B, H, W, C = x.shape
    xp = np.full((B, H + top + bottom, W + left + right, C), value, x.dtype)
    xp[:, top:top + H, left:left + W] = x
    return xp


def maxpool_same(x, rows=None):
    """ MaxPooling2D(3, strides 2, padding 'same') as TensorFlow pads: out = ceil(n / 2), pad_total = max((out - 1) 2 + 3 - n, 0),
    pad_before = pad_total // 2, and the padding never wins (-inf).  rows = (r0, r1): only output rows r0 .. r1 - 1 (a large map,
    compared in chunks) """
    x = np.asarray(x)
    _, H, W, _ = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pt, pl = max((Ho - 1) * 2 + 3 - H, 0), max((Wo - 1) * 2 + 3 - W, 0)
    r0, r1 = (0, Ho) if rows is None else rows
    lo, hi = 2 * r0 - pt // 2, 2 * (r1 - 1) + 3 - pt // 2             # the input rows under these output rows
    sub = x[:, max(lo, 0):min(hi, H)]
    return _window_max(_padded(sub, max(-lo, 0), max(hi - H, 0), pl // 2, pl - pl // 2, -np.inf), r1 - r0, Wo)


def maxpool_pad(x, pad):
    """ symmetric explicit padding of `pad` pixels + MaxPooling2D(3, strides 2, 'valid'): out = (n + 2 pad - 3) // 2 + 1; the padding
    never wins (-inf, the contract of gpp_maxpool3x3s2_pad_f32 in include/gpp.h) """
    x = np.asarray(x)
    _, H, W, _ = x.shape
    Ho, Wo = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1
    return _window_max(_padded(x, pad, pad, pad, pad, -np.inf), Ho, Wo)


def avgpool2x2(x):
    """ AveragePooling2D(2, strides 2, 'valid'): out = n // 2 (an odd last row / column is dropped); in float32, the window summed in
    row-major order, ((x00 + x01) + x10) + x11, then * 0.25 -- the order include/gpp.h states, so the result is defined to the bit """
    x = np.asarray(x, np.float32)
    _, H, W, _ = x.shape
    Ho, Wo = H // 2, W // 2
    a, b = x[:, 0:2 * Ho:2, 0:2 * Wo:2], x[:, 0:2 * Ho:2, 1:2 * Wo:2]
    c, d = x[:, 1:2 * Ho:2, 0:2 * Wo:2], x[:, 1:2 * Ho:2, 1:2 * Wo:2]
    return (((a + b).astype(np.float32) + c).astype(np.float32) + d).astype(np.float32) * np.float32(0.25)


# --------------------------------------------------------------------------------------------------------------- ReLU
def relu_words(raw, bits):
    """ ReLU on the raw words of an IEEE-like type whose top bit is the sign (bits = 16: f16 and bf16, 32: float32): a word with the sign
    set and a non-zero magnitude (negative numbers, negative subnormals, -inf) becomes +0; every other word is unchanged.  -0.0 is
    returned unchanged here: max(-0, +0) may be either zero, and the tests accept both for that one input. """
    raw = np.asarray(raw, {16: np.uint16, 32: np.uint32}[bits])
    sign = raw.dtype.type(1 << (bits - 1))
    negative = ((raw & sign) != 0) & ((raw & ~sign) != 0)
    return np.where(negative, raw.dtype.type(0), raw)


def relu_split_halves(raw_hi, raw_lo):
    """ ReLU on a pre-split x3 map, on the raw 16-bit words of the pairs (value = hi + lo, |lo| <= ulp(hi) / 2, so the sign of the value
    is the sign of hi): a pair whose hi is negative and non-zero becomes (+0, +0); every other pair -- hi = -0.0, hi > 0 with any lo --
    is unchanged.  The rule reads only the sign and magnitude bits, which f16 and bf16 keep in the same places. """
    hi, lo = np.asarray(raw_hi, np.uint16), np.asarray(raw_lo, np.uint16)
    negative = ((hi & np.uint16(0x8000)) != 0) & ((hi & np.uint16(0x7FFF)) != 0)
    return np.where(negative, np.uint16(0), hi), np.where(negative, np.uint16(0), lo)


# ----------------------------------------------------------------------------------------------------- weight packers
def packed_rows():
    """ channel held by packed row pos: row 16 h + 4 q + r of a group of 32 holds channel 8 q + 4 h + r of that group """
    rows = np.empty(64, np.int64)
    for g in range(2):
        for h in range(2):
            for q in range(4):
                for r in range(4):
                    rows[32 * g + 16 * h + 4 * q + r] = 32 * g + 8 * q + 4 * h + r
    return rows


def _packed_k(w_nk):
    """ (64 channels, 147) in (kh, kw, c) order -> (64, 232): k = kh * 32 + kw * 3 + c, every other slot zero """
    out = np.zeros((64, STEM_PITCH), w_nk.dtype)
    for kh in range(7):
        out[:, kh * 32:kh * 32 + 21] = w_nk[:, kh * 21:(kh + 1) * 21]
    return out


def pack_f16(w):
    """ gpp_stem_pack_weights_f16: w (147, 64) float32, k = (kh * 7 + kw) * 3 + c -> (64, 232) float16 (round to nearest even) """
    w = np.asarray(w, np.float32).reshape(147, 64)
    with np.errstate(over='ignore'):                 # a weight beyond 65504 is +-inf in f16: a plain cast, by definition
        return _packed_k(w.T[packed_rows()]).astype(np.float16)


def x3_exponent(amax):
    """ e with amax * 2^e in [2^13, 2^14) (0 for an all-zero channel), bounded to [X3_EXP_MIN, X3_EXP_MAX] so that the scale 2^e and its
    inverse 2^-e are both normal float32 numbers.  A float32 amax needs e in [-114, 162]: only the upper bound ever acts. """
    if not amax > 0:
        return 0
    _, ex = np.frexp(np.float64(amax))               # amax = m 2^ex, m in [0.5, 1)
    return int(min(max(14 - int(ex), X3_EXP_MIN), X3_EXP_MAX))


def pack_f16x3(w):
    """ gpp_stem_pack_weights_f16x3: w (147, 64) float32 -> (hi (64, 232) float16, lo (64, 232) float16, out_scale (64,) float32).
    Channel n is multiplied by 2^e(n) in float32, hi = f16(v), lo = f16(v - hi) (float32 subtraction: exact); rows and k as pack_f16;
    out_scale is indexed by CHANNEL (not by packed row) and is exactly 2^-e(n). """
    w = np.asarray(w, np.float32).reshape(147, 64)
    e = np.array([x3_exponent(np.abs(w[:, n]).max()) for n in range(64)])
    scale = np.ldexp(np.float64(1.0), e).astype(np.float32)
    out_scale = np.ldexp(np.float64(1.0), -e).astype(np.float32)
    with np.errstate(over='ignore', under='ignore'):
        v = _packed_k((w * scale[None, :]).astype(np.float32).T[packed_rows()])
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi, lo, out_scale


def pack_f16x3_bytes(w):
    """ the blob of gpp_stem_pack_weights_f16x3: [hi][lo][out_scale], 2 * 64 * 232 * 2 + 64 * 4 = 59 648 bytes """
    hi, lo, out_scale = pack_f16x3(w)
    return hi.tobytes() + lo.tobytes() + out_scale.tobytes()
