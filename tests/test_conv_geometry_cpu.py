"""
Convolution geometries beyond square 1 x 1 / 3 x 3 (gpp_conv2d_igemm accepts KH, KW in 1..8, any pad_top / pad_left, stride 1 or 2 and any
caller-chosen H_out / W_out): the case table that tests/test_conv_geometry_gpu.py runs on a device, and everything about it that needs none.

  * The table can fail.  For every case four (five) wrong float64 references -- kernel taps transposed (a KW x KH kernel: kh and kw swapped in
    offset and mask), the tap walk swapped over the same weights (kh inner instead of kw; identical for a 1 x N kernel, so KH, KW > 1 only),
    pad_top off by one, pad_left off by one, the last tap dropped -- each differ from the true one by more than the LOOSEST bar of the GPU
    file (bf16: 2^-8 |ref| + 1e-3) on at least a tenth of the outputs: a kernel with such a fault cannot pass there.  The all-padding rows of
    3x5_overhang are relu(bias) in the true reference and not with pad_top off by one.
    (One exception, asserted as such: on the 3 x 2 map of 7x7_tiny_map tap (6, 6) of the 7 x 7 / pad 3 kernel lands on no pixel at all, so a
    dropped last tap is invisible there.  7x7_small_map is the same layer on 6 x 5 -- still smaller than the kernel, every pixel a border
    pixel -- where it is not.)
  * layers/conv.pack_weight for rectangular kernels: an independent restatement of include/gpp.h's layout in plain loops (inverse of the row
    interleave, then K = (chunk, kh, kw, channel in chunk), [32 hi | 32 lo] halves per K-step for the x3 types) times an im2col of the
    input in the same K order, in float64, equals the float64 convolution -- within the weights' rounding to the type (a bound computed
    from |x| |w|), and with exactly the original weights for GPP_F32.
  * the entry points that need no device, on the new geometries: gpp_conv2d_flops, gpp_conv2d_split_rule, gpp_conv2d_workspace_bytes,
    gpp_conv2d_tile_candidates; KH = 9 / KW = 9 answer GPP_ERR_UNSUPPORTED.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C

DTYPES = ('bf16', 'f16', 'f32', 'bf16x3', 'f16x3')
UNSUPPORTED = -4

# name, B, H, W, C_in, C_out, (KH, KW), stride, pad (t, l) | None = TF 'same', out (h, w) | None = the input's size, relu,
# float32 output for the 16-bit types, what it reaches
GEOMETRY_CASES = [
    ('5x5_same', 2, 11, 13, 64, 96, (5, 5), 1, (2, 2), None, True, False),               # mask bits 3..4
    ('7x7_s2_tfsame', 1, 15, 22, 64, 128, (7, 7), 2, None, None, False, False),          # odd / even pad, deep tap walk; K = 3136
    ('1x7', 2, 9, 17, 64, 128, (1, 7), 1, (0, 3), None, True, False),                    # KH = 1: kh wraps on every step
    ('7x1', 2, 17, 9, 64, 64, (7, 1), 1, (3, 0), None, False, True),                     # KW = 1: kw wraps on every step
    ('8x1_pad7', 2, 6, 5, 64, 64, (8, 1), 1, (7, 0), (13, 5), False, False),             # bit 7 the only valid row bit at oy = 0
    ('1x8_pad7', 1, 5, 6, 64, 80, (1, 8), 1, (0, 7), (5, 13), True, True),               # bit 15 likewise
    ('8x8', 1, 10, 12, 64, 144, (8, 8), 1, (4, 3), None, True, True),                    # largest kernel, asymmetric pad; K = 4096
    ('2x2_s2_valid', 2, 12, 14, 64, 64, (2, 2), 2, (0, 0), (6, 7), False, False),        # even kernel, no border
    ('4x6_s2', 2, 13, 11, 64, 96, (4, 6), 2, (1, 4), (7, 6), False, False),              # even, rectangular, pad > K / 2 on one axis
    ('3x3_valid', 1, 9, 11, 64, 128, (3, 3), 1, (0, 0), (7, 9), True, False),            # output smaller than input
    ('3x3_full', 2, 7, 9, 64, 64, (3, 3), 1, (2, 2), (9, 11), False, True),              # corner outputs see exactly one tap
    ('3x5_overhang', 2, 6, 8, 64, 144, (3, 5), 1, (1, 2), (9, 8), True, True),           # output rows 7, 8 lie in the padding: relu(bias)
    ('7x7_tiny_map', 2, 3, 2, 64, 96, (7, 7), 1, (3, 3), None, False, False),            # map smaller than the kernel: every pixel is border
    ('7x7_small_map', 2, 6, 5, 64, 96, (7, 7), 1, (3, 3), None, True, False),            # ... at a size where the last tap lands on the map
    ('5x3_slice_res', 2, 8, 10, 64, 128, (5, 3), 1, (2, 1), None, True, False),          # channel slice of a 192-wide map, gapped batch stride, shortcut
]
CASE_IDS = [c[0] for c in GEOMETRY_CASES]
SLICE_PITCH, SLICE_OFFSET, SLICE_GAP = 192, 64, 384          # 5x3_slice_res: in_pitch, first channel, elements between the images


def case_named(name):
    return [c for c in GEOMETRY_CASES if c[0] == name][0]


def widened(case, cout):
    return case[:5] + (cout,) + case[6:]


def geometry(case):
    """ (pad_top, pad_left, H_out, W_out) """
    _, _, H, W, _, _, (KH, KW), stride, pad, out_hw, _, _ = case
    if pad is None:
        oh, pt = C.same_pad(H, KH, stride)
        ow, pl = C.same_pad(W, KW, stride)
        return pt, pl, oh, ow
    oh, ow = out_hw if out_hw else (H, W)
    return pad[0], pad[1], oh, ow


def operands(case):
    """ float32 x (B, H, W, C_in), k HWIO, bias (non-zero), shortcut or None: the same draw wherever the case is used """
    name, B, H, W, Cin, Cout, (KH, KW), _, _, _, _, _ = case
    g = torch.Generator().manual_seed(sum(map(ord, name)) + Cout)
    x = torch.randn((B, H, W, Cin), generator=g)
    k = torch.randn((KH, KW, Cin, Cout), generator=g) * (2.0 / (KH * KW * Cin)) ** 0.5
    bias = torch.randn((Cout,), generator=g) * 0.1 + 0.05
    _, _, oh, ow = geometry(case)
    res = torch.randn((B, oh, ow, Cout), generator=g) if name == '5x3_slice_res' else None
    return x, k, bias, res


def reference64(x, k, bias, stride, pad_t, pad_l, oh, ow, relu, res):
    """ float64 convolution of explicitly padded operands: x (B, H, W, C_in), k HWIO -> (B, oh, ow, C_out) """
    B, H, W, _ = x.shape
    KH, KW = k.shape[:2]
    pad_b = max((oh - 1) * stride + KH - H - pad_t, 0)
    pad_r = max((ow - 1) * stride + KW - W - pad_l, 0)
    xp = F.pad(x.double().permute(0, 3, 1, 2), (pad_l, pad_r, pad_t, pad_b))
    y = F.conv2d(xp, k.double().permute(3, 2, 0, 1), bias.double(), stride=stride)[:, :, :oh, :ow].permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def true_reference(case, x=None, k=None, res=None):
    x0, k0, bias, res0 = operands(case)
    pt, pl, oh, ow = geometry(case)
    return reference64(x0 if x is None else x, k0 if k is None else k, bias, case[7], pt, pl, oh, ow, case[10], res0 if res is None else res)


# ---------------------------------------------------------------------------------------------- the table can fail
def mutants(case):
    x, k, bias, res = operands(case)
    KH, KW = case[6]
    pt, pl, oh, ow = geometry(case)
    stride, relu = case[7], case[10]
    out = {}
    if KH != KW:
        out['taps transposed'] = reference64(x, k.transpose(0, 1).contiguous(), bias, stride, pt, pl, oh, ow, relu, res)
        if KH > 1 and KW > 1:         # tap t of the packed order read as (kh, kw) = (t % KH, t / KH)
            swapped = k.reshape(KW, KH, k.shape[2], k.shape[3]).transpose(0, 1).contiguous()
            out['walk swapped'] = reference64(x, swapped, bias, stride, pt, pl, oh, ow, relu, res)
    out['pad_top + 1'] = reference64(x, k, bias, stride, pt + 1, pl, oh, ow, relu, res)
    out['pad_left + 1'] = reference64(x, k, bias, stride, pt, pl + 1, oh, ow, relu, res)
    dropped = k.clone()
    dropped[KH - 1, KW - 1] = 0.0
    out['last tap dropped'] = reference64(x, dropped, bias, stride, pt, pl, oh, ow, relu, res)
    return out


@pytest.mark.parametrize('case', GEOMETRY_CASES, ids=CASE_IDS)
def test_a_wrong_tap_walk_or_pad_would_miss_the_loosest_bar(case):
    ref = true_reference(case)
    tol = 2.0 ** -8 * ref.abs() + 1e-3                    # bf16's bar: the loosest of tests/test_conv_geometry_gpu.py
    wrong = mutants(case)
    assert len(wrong) >= (4 if case[6][0] != case[6][1] else 3)
    for name, mut in wrong.items():
        if case[0] == '7x7_tiny_map' and name == 'last tap dropped':
            assert torch.equal(mut, ref)                  # tap (6, 6) reads row oy + 3 >= 3 of a 3-row map: 7x7_small_map covers it
            continue
        share = float(((mut - ref).abs() > tol).double().mean())
        assert share >= 0.1, (case[0], name, share)


def test_the_table_is_what_the_geometry_tests_were_asked_for():
    names = set(CASE_IDS)
    assert len(names) == len(GEOMETRY_CASES) == 15
    for case in GEOMETRY_CASES:
        _, B, H, W, Cin, Cout, (KH, KW), stride, _, _, _, _ = case
        assert Cin == 64 and 64 <= Cout <= 144 and B in (1, 2) and H * W <= 15 * 22 and KH * KW * Cin <= 4096
    assert {c[10] for c in GEOMETRY_CASES} == {True, False} and {c[11] for c in GEOMETRY_CASES} == {True, False}
    assert geometry(case_named('7x7_s2_tfsame')) == (3, 2, 8, 11)            # TF 'same' at stride 2: 6 rows of padding, 5 columns


def test_overhang_rows_are_relu_of_the_bias():
    case = case_named('3x5_overhang')
    _, _, bias, _ = operands(case)
    ref = true_reference(case)
    want = torch.relu(bias.double()).expand(ref.shape[0], 2, ref.shape[2], ref.shape[3])
    assert torch.equal(ref[:, 7:9], want)                  # output rows 7, 8 read input rows 6 .. 9 of a 6-row map
    assert float(want.max()) > 0.0 and not torch.equal(ref[:, 6:7], want[:, :1])
    shifted = mutants(case)['pad_top + 1']
    assert not torch.equal(shifted[:, 7:9], want)


# ---------------------------------------------------------------------------------------------- pack_weight, restated
def unpack_plain_loops(packed, dtype, KH, KW, Cin, Cout, scale=None):
    """ include/gpp.h's weight layout read back in plain loops: float64 (C_out, KH, KW, C_in) of the values the packed tensor holds """
    ck = 64 if dtype in ('bf16', 'f16') else 32
    ktot = KH * KW * Cin
    if dtype in C.X3_TYPES:
        halves = packed.contiguous().view(C.x3_half(dtype)).double().numpy()          # per K-step of 32 channels: [32 hi | 32 lo]
        assert halves.shape[1] == 2 * ktot
    else:
        plain = packed.double().numpy()
        assert plain.shape[1] == ktot
    out = np.zeros((Cout, KH, KW, Cin))
    for n in range(Cout):
        g, within = divmod(n, 32)
        q, h, r = within // 8, (within % 8) // 4, within % 4
        row = 32 * g + 16 * h + 4 * q + r                 # stored row 16 h + 4 q + r holds output channel 8 q + 4 h + r
        for chunk in range(Cin // ck):
            for kh in range(KH):
                for kw in range(KW):
                    step = (chunk * KH + kh) * KW + kw
                    if dtype in C.X3_TYPES:
                        v = halves[row, 64 * step:64 * step + 32] + halves[row, 64 * step + 32:64 * step + 64]
                        if scale is not None:
                            v = v * float(scale[n])
                    else:
                        v = plain[row, ck * step:ck * (step + 1)]
                    out[n, kh, kw, chunk * ck:(chunk + 1) * ck] = v
    return out


def im2col_plain_loops(x, KH, KW, stride, pt, pl, oh, ow):
    """ (B * oh * ow, KH, KW, C_in) float64: the input pixel under every tap of every output pixel, zeros outside the map """
    B, H, W, Cin = x.shape
    xs = x.double().numpy()
    out = np.zeros((B, oh, ow, KH, KW, Cin))
    for oy in range(oh):
        for kh in range(KH):
            iy = oy * stride - pt + kh
            if not 0 <= iy < H:
                continue
            for ox in range(ow):
                for kw in range(KW):
                    ix = ox * stride - pl + kw
                    if 0 <= ix < W:
                        out[:, oy, ox, kh, kw] = xs[:, iy, ix]
    return out.reshape(B * oh * ow, KH, KW, Cin)


# relative rounding of one weight on its way into the packed tensor: half an ulp of 8 (bf16) / 11 (f16) significant bits; for the x3 types
# that of the low half, itself at most half an ulp of the high one
WEIGHT_EPS = {'bf16': 2.0 ** -8, 'f16': 2.0 ** -11, 'f32': 0.0, 'bf16x3': 2.0 ** -16, 'f16x3': 2.0 ** -22}
# ... and the absolute one where a (half of a) weight can be a subnormal IEEE half: spacing 2^-24, for f16x3 under the channel's 2^13 .. 2^14 scale
WEIGHT_ABS = {'bf16': 0.0, 'f16': 2.0 ** -25, 'f32': 0.0, 'bf16x3': 0.0, 'f16x3': 2.0 ** -30}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['1x7', '7x1', '4x6_s2', '8x8'])
def test_pack_weight_orders_a_rectangular_kernel_as_the_header_says(name, dtype):
    case = widened(case_named(name), 40)                   # 40 output channels: one whole 32-row interleave group and a part of one
    _, B, H, W, Cin, Cout, (KH, KW), stride, _, _, _, _ = case
    x, k, bias, _ = operands(case)
    pt, pl, oh, ow = geometry(case)
    packed = C.pack_weight(k.numpy(), dtype, 'cpu')
    assert tuple(packed.shape) == (256, KH * KW * Cin)
    scale = C.out_scale_of(k.numpy(), 'cpu').double().numpy() if dtype == 'f16x3' else None
    held = unpack_plain_loops(packed, dtype, KH, KW, Cin, Cout, scale)
    want = k.double().permute(3, 0, 1, 2).numpy()
    if dtype == 'f32':
        assert np.array_equal(held, want)
    else:
        assert bool((np.abs(held - want) <= WEIGHT_EPS[dtype] * np.abs(want) + WEIGHT_ABS[dtype]).all())
        assert not np.array_equal(held, want)
    # the rows past C_out (up to the whole interleave group and on to 256) are zero
    used = set(32 * (n // 32) + 16 * ((n % 8) // 4) + 4 * ((n % 32) // 8) + n % 4 for n in range(Cout))
    rest = [r for r in range(256) if r not in used]
    assert not packed.view(torch.int32 if packed.element_size() == 4 else torch.int16)[rest].any()
    cols = im2col_plain_loops(x, KH, KW, stride, pt, pl, oh, ow).reshape(B * oh * ow, -1)
    got = cols @ held.reshape(Cout, -1).T + bias.double().numpy()
    ref = reference64(x, k, bias, stride, pt, pl, oh, ow, False, None).reshape(B * oh * ow, Cout).numpy()
    bound = WEIGHT_EPS[dtype] * (np.abs(cols) @ np.abs(want.reshape(Cout, -1)).T) + WEIGHT_ABS[dtype] * np.abs(cols).sum(axis=1)[:, None] + \
        1e-12 * (1.0 + np.abs(ref))
    assert bool((np.abs(got - ref) <= bound).all()), float(np.abs(got - ref).max())
    # ... and a transposed walk over the same packed values is not the convolution: the check above has teeth
    if KH > 1 and KW > 1:
        walked = held.reshape(Cout, KH * KW, Cin).reshape(Cout, KW, KH, Cin).transpose(0, 2, 1, 3)
        bad = cols @ walked.reshape(Cout, -1).T + bias.double().numpy()
        assert float((np.abs(bad - ref) > 2.0 ** -8 * np.abs(ref) + 1e-3).mean()) > 0.1


# ---------------------------------------------------------------------------------------------- entry points that need no device
def host_desc(case, dtype, tile=0, workspace=None, split_k=0, batch=None):
    """ a descriptor over host tensors: for the entry points that never launch """
    _, B, H, W, Cin, Cout, (KH, KW), stride, _, _, relu, out_f32 = case
    B = batch or B
    pt, pl, oh, ow = geometry(case)
    tdt = C.torch_dtype(dtype)
    k = torch.zeros((KH, KW, Cin, Cout)).numpy()
    keep = [C.FMap.empty(B, H, W, Cin, tdt, 'cpu'), C.FMap.empty(B, oh, ow, Cout, torch.float32 if out_f32 else tdt, 'cpu'),
            C.pack_weight(k, dtype, 'cpu'), torch.zeros((Cout,)), C.out_scale_of(k, 'cpu') if dtype == 'f16x3' else None, workspace]
    d = C.conv_desc([keep[0]], [keep[1]], keep[2], keep[3], KH, KW, Cin, Cout, stride=stride, pad=(pt, pl), relu=relu, dtype=dtype,
                    out_f32=out_f32 and dtype in ('bf16', 'f16'), tile_hint=tile, workspace=workspace, split_k=split_k, out_scale=keep[4])
    return d, keep


@pytest.mark.parametrize('case', GEOMETRY_CASES, ids=CASE_IDS)
def test_device_free_entry_points_on_the_new_geometries(case):
    name, B, H, W, Cin, Cout, (KH, KW), stride, _, _, _, _ = case
    _, _, oh, ow = geometry(case)
    ws = torch.empty((1 << 20,), dtype=torch.uint8)
    for dtype in DTYPES:
        d, keep = host_desc(case, dtype)
        assert abs(C.conv_flops(d) - 2.0 * B * oh * ow * KH * KW * Cin * Cout) < 1.0
        tiles, count = (ctypes.c_int * 64)(), ctypes.c_int(0)
        hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(d), tiles, 64, ctypes.byref(count)), 'gpp_conv2d_tile_candidates')
        assert 1 <= count.value <= 64 and tiles[0] == 0 and len(set(tiles[:count.value])) == count.value
        assert C.split_rule(d) == 1                          # no workspace: never split
        # K = 3136 (7 x 7) and 4096 (8 x 8) on a grid of one or two tiles per image: (K + 768) / 1536; every other case is shallower than 3072
        want = {'7x7_s2_tfsame': 2, '7x7_tiny_map': 2, '7x7_small_map': 2, '8x8': 3}.get(name, 1)
        for batch in (1, 2, 8):
            for tile in (0, 64128, 128128, 224128):
                dw, keep_w = host_desc(case, dtype, tile=tile, workspace=ws, batch=batch)
                assert C.split_rule(dw) == want, (dtype, batch, tile)
                need = C.workspace_bytes(dw)
                if want == 1:
                    assert need == 0
                    continue
                # the float32 partial slabs of that factor for every block tile the library has: rows and columns rounded up to the tile
                for bm, bn in ((64, 64), (128, 128), (224, 128), (192, 160), (256, 256), (96, 64)):
                    assert need >= want * (-(-batch * oh * ow // bm) * bm) * (-(-Cout // bn) * bn) * 4, (dtype, batch, bm, bn)


@pytest.mark.parametrize('kh,kw', [(9, 1), (1, 9), (9, 9), (3, 9)])
def test_kernels_beyond_eight_taps_a_side_are_refused(kh, kw):
    for dtype in DTYPES:
        d, keep = host_desc(case_named('3x3_valid'), dtype)
        d.KH, d.KW = kh, kw
        lib = hip.lib()
        k, n = ctypes.c_int(0), hip.c_size_t(0)
        tiles, count = (ctypes.c_int * 64)(), ctypes.c_int(0)
        assert lib.gpp_conv2d_split_rule(ctypes.byref(d), ctypes.byref(k)) == UNSUPPORTED
        assert lib.gpp_conv2d_workspace_bytes(ctypes.byref(d), ctypes.byref(n)) == UNSUPPORTED
        assert lib.gpp_conv2d_tile_candidates(ctypes.byref(d), tiles, 64, ctypes.byref(count)) == UNSUPPORTED
        assert lib.gpp_conv2d_igemm(ctypes.byref(d), None) == UNSUPPORTED          # (refused by the validator, before any launch)
    d, keep = host_desc(case_named('8x8'), 'f32')
    assert C.split_rule(d) == 1                                                     # 8 x 8 is inside
