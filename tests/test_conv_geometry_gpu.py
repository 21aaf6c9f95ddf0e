"""
gpp_conv2d_igemm on the geometries its validator accepts and no network here uses: kernels up to 8 x 8, rectangular and even ones, pads beyond
K / 2 and asymmetric ones, caller-chosen output sizes (rows that lie wholly in the padding), maps smaller than the kernel -- the table of
tests/test_conv_geometry_cpu.py, which also shows (without a device) that a swapped tap walk, a pad off by one or a dropped tap would miss the
loosest bar used here.

Reference: a float64 convolution on the CPU of the values the operands hold (rounded to the type for GPP_BF16 / GPP_F16, the hi + lo a
pre-split map keeps for the x3 types), explicitly padded.  Bars: the project's own, as stated in the files that own them --

    GPP_BF16 / GPP_F16   |err| <= eps |ref| + 1e-3, eps = 2^-8 / 2^-10                          (tests/test_conv_gpu.py)
    GPP_F32              |err| <= 1e-5 |ref| + 2e-6 rms(ref) sqrt(K)                            (tests/test_conv_f32_gpu.py)
    GPP_BF16X3           |err| <= 1e-4 |ref| + 1e-4 rms(ref)                                    (tests/test_conv_f32_gpu.py)
    GPP_F16X3            float32's bar, and rms(err) <= (3e-8 sqrt(K) + 1e-7) rms(ref)          (tests/test_conv_f16x3_gpu.py)

K is at most 4096 here.  Every test prints its worst err / tol; test_zz_the_worst_ratio_of_every_type prints the worst per type of the run.

Per case and type: the default tile meets the bar (output pre-filled with NaN); every explicit tile the type owns gives the default's bits,
and a form the type or input form does not have is REFUSED (GPP_ERR_UNSUPPORTED), not skipped; split-K 2 / 3 / 5 with a workspace meets the bar
with the same bits from different tiles, and the library's own rule gives the bytes of its factor run explicitly; the dual-shape and the
mixed-height grids give the bits of the plain 128 x 128 tile on a rectangular kernel; the gathered forms write the dense launch's rows at
the listed pixels (border pixels and a random third of the rest, in shuffled order) and nothing else; the autotuner returns a listed tile.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from test_conv_gpu import ALL_TILES
from test_conv_f32_gpu import F32_TILES, X3_TILES, X3_F32IN_TILES, _x3_round
from test_conv_f16x3_gpu import PLAIN_TILES, PIPE_TILES, DEEP_TILES, held
from test_conv_geometry_cpu import (GEOMETRY_CASES, CASE_IDS, DTYPES, SLICE_PITCH, SLICE_OFFSET, SLICE_GAP, case_named, widened, geometry,
                                    operands, reference64)

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -4
POISON = 0x7fc0dead                                   # a quiet NaN no kernel produces (as a pair of halves: a NaN beside a value nobody stores)
GATHER_TILES = (6064064, 7032064, 6064160)
WORST = {}                                            # type -> (worst err / tol, where)

# the explicit tile codes of a type and input form: (those that run, those refused as GPP_ERR_UNSUPPORTED for their documented reason)
assert sorted(X3_F32IN_TILES) == sorted(PLAIN_TILES) and sorted(X3_TILES) == sorted(PLAIN_TILES + [192160])
SPLIT_INPUT_ONLY = [192160] + PIPE_TILES + DEEP_TILES                  # x3 types: these forms read pre-split rows
F32_HAS_NOT = [256256, 1128128, 1192256, 2256256, 128256, 5064064]     # 16-bit / x3 forms: float32 has no instantiation


def tiles_of(dtype, flags):
    if dtype in ('bf16', 'f16'):
        return ALL_TILES, []
    if dtype == 'f32':
        return F32_TILES, F32_HAS_NOT
    return (PLAIN_TILES + SPLIT_INPUT_ONLY, []) if flags & 1 else (PLAIN_TILES, SPLIT_INPUT_ONLY)


def forms_of(dtype):
    """ x3_split flags to run a type with: float32 maps, pre-split input, pre-split input and output """
    return (0, 1, 3) if dtype in C.X3_TYPES else (0,)


def launch(d):
    return hip.lib().gpp_conv2d_igemm(ctypes.byref(d), hip.stream_ptr())


class Layer(object):
    """ one case of the table on the device in one element type and map form, with its float64 reference """

    def __init__(self, case, dtype, flags):
        name, B, H, W, Cin, Cout, (KH, KW), stride, _, _, relu, out_f32 = case
        dev = torch.device('cuda')
        self.case, self.dtype, self.flags, self.kdepth = case, dtype, flags, KH * KW * Cin
        self.geom = geometry(case)
        pt, pl, oh, ow = self.geom
        x, k, bias, res = operands(case)
        tdt = C.torch_dtype(dtype)
        x3 = dtype in C.X3_TYPES
        if not x3:                                    # operands rounded to the storage type first (a no-op for float32)
            x, k, res = x.to(tdt).float(), k.to(tdt).float(), None if res is None else res.to(tdt).float()
        keeps = held if dtype == 'f16x3' else _x3_round
        x_held = keeps(x) if flags & 1 else x
        self.ref = reference64(x_held, k, bias, stride, pt, pl, oh, ow, relu, res)
        self.rms = float(self.ref.pow(2).mean().sqrt())
        half = dtype if x3 else 'bf16x3'
        if name == '5x3_slice_res':                   # channels 64 .. 127 of a 192-channel map, images SLICE_GAP elements apart; NaN all around
            bstride = H * W * SLICE_PITCH + SLICE_GAP
            buf = torch.full((B * bstride,), float('nan'), dtype=tdt, device=dev)
            self.xin = C.FMap(buf, B, H, W, Cin, off=SLICE_OFFSET, bstride=bstride, pitch=SLICE_PITCH, split=bool(flags & 1), half=half)
        else:
            self.xin = C.FMap.empty(B, H, W, Cin, tdt, dev, split=bool(flags & 1), half=half)
        self.xin.write(x)
        self.out_f32 = bool(out_f32) and not x3 and dtype != 'f32'
        self.out = C.FMap.empty(B, oh, ow, Cout, torch.float32 if self.out_f32 else tdt, dev, split=bool(flags & 2), half=half)
        self.out32 = C.FMap.empty(B, oh, ow, Cout, torch.float32, dev)                 # the gathered forms write float32
        self.rmap = None
        if res is not None:
            rm = C.FMap.empty(B, oh, ow, Cout, tdt, dev)
            rm.write(res)
            self.rmap = [rm]
        self.w = C.pack_weight(k.numpy(), dtype, dev)
        self.scale = C.out_scale_of(k.numpy(), dev) if dtype == 'f16x3' else None
        self.bias = bias.to(dev)
        self.ws = workspace()
        self.rows = torch.zeros((B * oh * ow,), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((hip.GPP_MAX_GROUPS + 1,), dtype=torch.int32, device=dev)

    def make(self, tile=0, split_k=1, workspace=False, gathered=False, f32=False):
        _, _, _, _, Cin, Cout, (KH, KW), stride, _, _, relu, _ = self.case
        d = C.conv_desc([self.xin], [self.out32 if f32 else self.out], self.w, self.bias, KH, KW, Cin, Cout, stride=stride, pad=self.geom[:2],
                        relu=relu, residuals=self.rmap, dtype=self.dtype, out_f32=self.out_f32 or f32, tile_hint=tile,
                        workspace=self.ws if workspace else None, split_k=split_k, out_scale=self.scale)
        if gathered:
            d.gather_rows, d.gather_counts = self.rows.data_ptr(), self.counts.data_ptr()
        return d

    def poison(self, f32=False):
        (self.out32 if f32 else self.out).buf.fill_(float('nan'))

    def bits(self, f32=False):
        buf = (self.out32 if f32 else self.out).buf
        return buf.view(torch.int32 if buf.element_size() == 4 else torch.int16).clone()

    def check(self, what):
        """ the output map against the float64 reference with the type's bar; returns (and records) the worst err / tol """
        got = self.out.read().double().cpu()
        assert torch.isfinite(got).all(), what
        err = (got - self.ref).abs()
        if self.dtype in ('bf16', 'f16'):
            tol = (2.0 ** -8 if self.dtype == 'bf16' else 2.0 ** -10) * self.ref.abs() + 1e-3
        elif self.dtype == 'bf16x3':
            tol = 1e-4 * self.ref.abs() + 1e-4 * self.rms
        else:
            tol = 1e-5 * self.ref.abs() + 2e-6 * self.rms * self.kdepth ** 0.5
        ratio = float((err / tol).max())
        if self.dtype == 'f16x3':
            ratio = max(ratio, float(err.pow(2).mean().sqrt()) / ((3e-8 * self.kdepth ** 0.5 + 1e-7) * self.rms))
        where = '{} {} x3_split={} {}'.format(self.case[0], self.dtype, self.flags, what)
        print('err / tol = {:.3f}  {}'.format(ratio, where))
        if ratio > WORST.get(self.dtype, (0.0, ''))[0]:
            WORST[self.dtype] = (ratio, where)
        assert ratio <= 1.0, (where, ratio, float(err.max()))
        return ratio

    def put_rows(self, rows):
        buf = np.zeros((self.rows.numel(),), np.int32)
        buf[:len(rows)] = rows
        self.rows.copy_(torch.as_tensor(buf))
        self.counts.copy_(torch.as_tensor([len(rows)] + [0] * (hip.GPP_MAX_GROUPS - 1) + [len(rows)], dtype=torch.int32))


_LAYERS, _WS = {}, []


def workspace():
    if not _WS:
        _WS.append(torch.empty((32 << 20,), dtype=torch.uint8, device='cuda'))
    return _WS[0]


def layer(case, dtype, flags=0):
    key = (case[0], case[5], dtype, flags)
    if key not in _LAYERS:
        _LAYERS[key] = Layer(case, dtype, flags)
    return _LAYERS[key]


def split_output_is_refused(case, dtype, flags):
    """ a pre-split output holds whole 32-channel blocks: the validator refuses other widths """
    if not (flags & 2) or case[5] % 32 == 0:
        return False
    _, B, H, W, Cin, Cout, (KH, KW), stride, _, _, relu, _ = case
    pt, pl, oh, ow = geometry(case)
    dev = torch.device('cuda')
    x = C.FMap.empty(B, H, W, Cin, torch.float32, dev, split=True, half=dtype)
    o = C.FMap.empty(B, oh, ow, Cout, torch.float32, dev)
    k = torch.zeros((KH, KW, Cin, Cout)).numpy()
    keep = (C.pack_weight(k, dtype, dev), C.out_scale_of(k, dev) if dtype == 'f16x3' else None)
    d = C.conv_desc([x], [o], keep[0], None, KH, KW, Cin, Cout, stride=stride, pad=(pt, pl), dtype=dtype, out_scale=keep[1])
    d.x3_split = 3
    assert launch(d) == UNSUPPORTED
    return True


# ---------------------------------------------------------------------------------------------- 1, 2: the default tile, every tile
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', GEOMETRY_CASES, ids=CASE_IDS)
def test_default_tile_meets_the_bar_and_every_tile_gives_its_bits(case, dtype):
    for flags in forms_of(dtype):
        if split_output_is_refused(case, dtype, flags):
            continue
        L = layer(case, dtype, flags)
        L.poison()
        C.run_conv(L.make(0))
        L.check('default tile')
        base = L.bits()
        runs, refused = tiles_of(dtype, flags)
        for tile in runs:
            d = L.make(tile)
            bn = tile % 1000
            if -(-d.C_out // bn) * bn > d.weight_rows:              # the tile grid would read past the packed weight rows
                assert launch(d) == BAD_ARG
                continue
            L.poison()
            rc = launch(d)
            assert rc == 0, (tile, flags, rc)
            assert torch.equal(L.bits(), base), (tile, flags)
        for tile in refused:
            assert launch(L.make(tile)) == UNSUPPORTED, (tile, flags)


# ---------------------------------------------------------------------------------------------- 3: split-K inside a rectangular tap grid
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['7x7_s2_tfsame', '4x6_s2', '1x7', '8x8'])
def test_split_k_restarts_inside_the_tap_grid(name, dtype):
    """ K-steps (16-bit types; twice as many for the float32-sized ones): 49, 24, 7, 64 -- the splits start mid-row and mid-grid of the kernel """
    case = case_named(name)
    for flags in forms_of(dtype)[:2]:
        L = layer(case, dtype, flags)
        others = [192128]
        if dtype in ('bf16', 'f16') or flags & 1:
            others += [1128128, 1192096]                           # the pipelined loops restart from their own copy of the walk
        if flags & 1:
            others += [5064128, 1256256]                           # ... and so does the four-deep ring
        for split in (2, 3, 5):
            L.poison()
            C.run_conv(L.make(64128, split_k=split, workspace=True))
            L.check('split_k={}'.format(split))
            first = L.bits()
            for tile in others:
                L.poison()
                C.run_conv(L.make(tile, split_k=split, workspace=True))
                assert torch.equal(L.bits(), first), (tile, split, flags)
        if name == '7x7_s2_tfsame':                                # K = 3136 on a one-tile grid: the library's rule says 2
            d = L.make(0, split_k=0, workspace=True)
            assert C.split_rule(d) == 2
            L.poison()
            C.run_conv(d)
            L.check('split_k=0 (the rule)')
            ruled = L.bits()
            L.poison()
            C.run_conv(L.make(0, split_k=2, workspace=True))
            assert torch.equal(L.bits(), ruled)
            L.poison()
            C.run_conv(L.make(0, split_k=0))                       # without a workspace the rule never splits: the unsplit bits
            unsplit = L.bits()
            L.poison()
            C.run_conv(L.make(0, split_k=1, workspace=True))
            assert torch.equal(L.bits(), unsplit)


# ---------------------------------------------------------------------------------------------- 4: the dual-shape and mixed-height grids
@pytest.mark.parametrize('dtype', ['bf16', 'f16', 'bf16x3', 'f16x3'])
def test_dual_shape_grid_on_a_5x5_kernel(dtype):
    """ 2256256 (C_out = 384: a 256-column part and a 512 x 128 part whose tap offsets are formed when a piece is issued) against 128128 """
    flags = 3 if dtype in C.X3_TYPES else 0
    L = layer(widened(case_named('5x5_same'), 384), dtype, flags)
    L.poison()
    C.run_conv(L.make(128128))
    L.check('128128 at C_out = 384')
    base = L.bits()
    L.poison()
    C.run_conv(L.make(2256256))
    assert torch.equal(L.bits(), base)
    if flags:                                                      # float32 input map: the dual grid (a pipelined form) is refused
        assert launch(layer(widened(case_named('5x5_same'), 384), dtype, 0).make(2256256)) == UNSUPPORTED
    else:                                                          # a single K-step (1 x 1, 64 channels): nk < 2, refused
        dev = torch.device('cuda')
        tdt = C.torch_dtype(dtype)
        keep = (C.FMap.empty(1, 4, 4, 64, tdt, dev), C.FMap.empty(1, 4, 4, 384, tdt, dev), C.pack_weight(torch.zeros((1, 1, 64, 384)).numpy(), dtype, dev))
        d = C.conv_desc([keep[0]], [keep[1]], keep[2], None, 1, 1, 64, 384, dtype=dtype, tile_hint=2256256)
        assert launch(d) == UNSUPPORTED


@pytest.mark.parametrize('tile', [3256224, 3192160])
@pytest.mark.parametrize('kernel', [(1, 7), (3, 5)], ids=['1x7', '3x5'])
@pytest.mark.parametrize('dtype', ['bf16x3', 'f16x3'])
def test_mixed_height_grid_on_a_rectangular_kernel(dtype, kernel, tile):
    """ the mixed grids take a layer only where a whole round of 256 workgroups fits its first map: the table's 1x7 at C_out = 256 is
    declined (GPP_ERR_UNSUPPORTED), the same kernel on a 2 x 187 x 181 map runs -- the bits of 128128, which is held to the float64
    reference on a sample of its pixels.  (A 1 x N kernel is walked the same way whichever of kh / kw is the inner one: 3 x 5, pad (1, 2),
    is here for that.) """
    assert launch(layer(widened(case_named('1x7'), 256), dtype, 3).make(tile)) == UNSUPPORTED
    B, H, W, Cin, Cout = 2, 187, 181, 64, 256
    KH, KW = kernel
    pt, pl = KH // 2, KW // 2
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(tile % 1000 + KH)
    x = torch.randn((B, H, W, Cin), generator=g)
    k = torch.randn((KH, KW, Cin, Cout), generator=g) * (2.0 / (KH * KW * Cin)) ** 0.5
    bias = torch.randn((Cout,), generator=g) * 0.1 + 0.05
    xin = C.FMap.empty(B, H, W, Cin, torch.float32, dev, split=True, half=dtype)
    xin.write(x)
    out = C.FMap.empty(B, H, W, Cout, torch.float32, dev, split=True, half=dtype)
    keep = (C.pack_weight(k.numpy(), dtype, dev), C.out_scale_of(k.numpy(), dev) if dtype == 'f16x3' else None, bias.to(dev))

    def run(code):
        out.buf.fill_(float('nan'))
        d = C.conv_desc([xin], [out], keep[0], keep[2], KH, KW, Cin, Cout, pad=(pt, pl), relu=True, dtype=dtype, tile_hint=code, out_scale=keep[1])
        rc = launch(d)
        assert rc == 0, (code, rc)
        return out.buf.view(torch.int32).clone()
    base = run(128128)
    values = out.read().double().cpu()
    assert torch.isfinite(values).all()
    # float64 on 600 random pixels and the four corners: the taps of a pixel from the zero-padded map
    rng = np.random.default_rng(tile)
    b = torch.as_tensor(np.concatenate([rng.integers(0, B, 600), [0, 0, B - 1, B - 1]]))
    oy = torch.as_tensor(np.concatenate([rng.integers(0, H, 600), [0, 0, H - 1, H - 1]]))
    ox = torch.as_tensor(np.concatenate([rng.integers(0, W, 600), [0, W - 1, 0, W - 1]]))
    xp = F.pad((held if dtype == 'f16x3' else _x3_round)(x).double(), (0, 0, pl, KW - 1 - pl, pt, KH - 1 - pt))
    patches = torch.stack([xp[b, oy + kh, ox + kw] for kh in range(KH) for kw in range(KW)], dim=1).reshape(len(b), KH * KW * Cin)
    ref = torch.relu(patches @ k.double().reshape(KH * KW * Cin, Cout) + bias.double())
    err = (values[b, oy, ox] - ref).abs()
    rms = float(ref.pow(2).mean().sqrt())
    tol = 1e-4 * ref.abs() + 1e-4 * rms if dtype == 'bf16x3' else 1e-5 * ref.abs() + 2e-6 * rms * (KH * KW * Cin) ** 0.5
    ratio = float((err / tol).max())
    print('err / tol = {:.3f}  {}x{} on 2 x 187 x 181, {} pre-split, 128128 (sampled)'.format(ratio, KH, KW, dtype))
    assert ratio <= 1.0
    assert torch.equal(run(tile), base)


# ---------------------------------------------------------------------------------------------- 5: the gathered forms
def listed_pixels(B, oh, ow, seed):
    """ every border pixel of every image and a random third of the rest, as b * H_out * W_out + p, in shuffled order """
    rng = np.random.default_rng(seed)
    edge = [y * ow + x for y in range(oh) for x in range(ow) if y in (0, oh - 1) or x in (0, ow - 1)]
    inner = sorted(set(range(oh * ow)) - set(edge))
    rows = []
    for b in range(B):
        rows += [b * oh * ow + p for p in edge]
        rows += [b * oh * ow + int(p) for p in rng.choice(inner, size=len(inner) // 3, replace=False)]
    return rng.permutation(rows).astype(np.int32)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['5x5_same', '1x7', '3x5_overhang'])
def test_gathered_rows_are_the_dense_rows(name, dtype):
    case = case_named(name)
    _, B, _, _, _, Cout, _, _, _, _, _, _ = case
    _, _, oh, ow = geometry(case)
    for flags in forms_of(dtype)[:2]:
        L = layer(case, dtype, flags)
        L.poison(f32=True)
        C.run_conv(L.make(0, f32=True))
        dense = L.bits(f32=True).reshape(B * oh * ow, Cout)
        assert torch.isfinite(L.out32.buf).all()
        rows = listed_pixels(B, oh, ow, seed=len(name) + flags)
        assert 0 < len(rows) < B * oh * ow and len(set(rows.tolist())) == len(rows)
        L.put_rows(rows)
        listed = torch.zeros((B * oh * ow,), dtype=torch.bool, device='cuda')
        listed[torch.as_tensor(rows.astype(np.int64), device='cuda')] = True
        want = torch.where(listed[:, None], dense, torch.full_like(dense, POISON))
        for tile in (0,) + GATHER_TILES:
            L.out32.buf.view(torch.int32).fill_(POISON)
            rc = launch(L.make(tile, gathered=True, f32=True))
            assert rc == 0, (tile, flags, rc)
            got = L.bits(f32=True).reshape(B * oh * ow, Cout)
            assert torch.equal(got, want), (tile, flags, int((got != want).sum()))


@pytest.mark.parametrize('dtype', ['bf16x3', 'f16x3'])
def test_gathered_rows_into_a_pre_split_map(dtype):
    """ 8000256 (the three-phase loop over the listed rows, height chosen on the device): 1x7 at C_out = 256, pre-split input and output """
    case = widened(case_named('1x7'), 256)
    _, B, _, _, _, Cout, _, _, _, _, _, _ = case
    _, _, oh, ow = geometry(case)
    L = layer(case, dtype, 3)
    L.poison()
    C.run_conv(L.make(0))
    L.check('dense, C_out = 256')
    dense = L.bits().reshape(B * oh * ow, Cout)
    rows = listed_pixels(B, oh, ow, seed=8)
    L.put_rows(rows)
    listed = torch.zeros((B * oh * ow,), dtype=torch.bool, device='cuda')
    listed[torch.as_tensor(rows.astype(np.int64), device='cuda')] = True
    want = torch.where(listed[:, None], dense, torch.full_like(dense, POISON))
    for tile in (8000256, 0, 8128256):
        L.out.buf.view(torch.int32).fill_(POISON)
        rc = launch(L.make(tile, gathered=True))
        assert rc == 0, (tile, rc)
        got = L.bits().reshape(B * oh * ow, Cout)
        assert torch.equal(got, want), (tile, int((got != want).sum()))


# ---------------------------------------------------------------------------------------------- 6: the autotuner
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['7x7_s2_tfsame', '1x7'])
def test_autotune_returns_a_listed_tile_that_meets_the_bar(name, dtype):
    for flags in forms_of(dtype)[::2]:                             # float32 maps; x3 types: pre-split input and output too
        L = layer(case_named(name), dtype, flags)
        d = L.make(0, split_k=0, workspace=True)
        tiles, count = (ctypes.c_int * 64)(), ctypes.c_int(0)
        hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(d), tiles, 64, ctypes.byref(count)), 'gpp_conv2d_tile_candidates')
        listed = list(tiles[:count.value])
        assert listed and listed[0] == 0
        best = ctypes.c_float(-1.0)
        hip.check(hip.lib().gpp_conv2d_autotune(ctypes.byref(d), 2, hip.stream_ptr(), ctypes.byref(best)), 'gpp_conv2d_autotune')
        assert d.tile_hint in listed and d.split_k == 0 and 0.0 < best.value < 1e5
        L.poison()
        C.run_conv(d)
        L.check('autotuned tile {}'.format(d.tile_hint))


def test_zz_the_worst_ratio_of_every_type():
    """ (runs last in the file) the measured worst err / tol per element type over whatever part of this file ran """
    for dtype in DTYPES:
        if dtype in WORST:
            print('worst err / tol  {:7s} {:.3f}  ({})'.format(dtype, *WORST[dtype]))
            assert WORST[dtype][0] <= 1.0
