"""
Sparse head outputs: the output layers of the regression and dimension towers evaluated only at the pixels the
decode reads.

  * kernel level -- the gathered-row form of gpp_conv2d_igemm (gpp_conv_desc.gather_rows): every listed row holds exactly the bytes of
    the dense launch, every other byte of the output map keeps the poison it was filled with, every gathered tile gives the same bytes,
    and a guarded launch (gpp_conv_desc.guard) does its work exactly when the device value matches;
  * the list kernels (gpp_detect_pixel_lists) against NumPy -- ascending lists that depend on the candidate set, not on the key order;
  * plan level -- GPP_SPARSE_HEADS=1 against 0: the same bytes in every output, and the head tensors read in full are the dense run's.

Byte equality throughout: a gathered row IS the dense row (same K order, same epilogue), so there is no tolerance to state.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from keras_retinanet_3D.utils import synthetic

pytestmark = pytest.mark.gpu

B = 2
LEVELS = [(13, 21), (7, 11), (4, 6)]
PIX = [h * w for h, w in LEVELS]
TOTAL = sum(PIX)
GATHER_TILES = (6064064, 6032064, 6064160, 7064064, 7032064, 7064160)       # 6 / 7000000 + BM * 1000 + BN: two- / four-deep ring (include/gpp.h)
POISON = 0x7fc0dead                              # a quiet NaN no kernel produces


def tiles_of(cout):
    return [t for t in GATHER_TILES if t % 1000 != 160 or -(-cout // 160) * 160 < -(-cout // 64) * 64]


def border(h, w):
    return sorted({y * w + x for y in range(h) for x in range(w) if y in (0, h - 1) or x in (0, w - 1)})


def pixel_lists():
    """ name -> per level the ascending list of b * H * W + p """
    rng = np.random.default_rng(7)
    every = [list(range(B * p)) for p in PIX]
    lists = {'empty': [[] for _ in PIX],
             'one pixel': [[5], [], []],
             'one pixel in the last level, last image': [[], [], [B * PIX[2] - 1]],
             'every pixel': every,
             'corners': [[b * h * w + p for b in range(B) for p in (0, w - 1, (h - 1) * w, h * w - 1)] for h, w in LEVELS],
             'borders': [[b * h * w + p for b in range(B) for p in border(h, w)] for h, w in LEVELS],
             'random 10 %': [sorted(rng.choice(B * p, size=max(1, B * p // 10), replace=False).tolist()) for p in PIX]}
    for bm in (32, 64):                           # the row counts around a tile of every instantiated height, in the first two levels
        for n in (bm - 1, bm, bm + 1):
            lists['{} rows'.format(n)] = [sorted(rng.choice(B * PIX[0], size=n, replace=False).tolist()),
                                          sorted(rng.choice(B * PIX[1], size=n, replace=False).tolist()), []]
    return lists


class Layer(object):
    """ one head output layer over the three levels: 3 x 3, pad 1, C_in -> C_out, float32 output; the dense result computed once """

    def __init__(self, dtype, split, cin, cout):
        dev = torch.device('cuda')
        g = torch.Generator().manual_seed(1000 * cin + cout)
        self.dtype, self.cout = dtype, cout
        tdt = C.torch_dtype(dtype)
        self.xbuf = torch.empty((B, TOTAL, cin), dtype=tdt, device=dev)
        self.obuf = torch.empty((B, TOTAL, cout), dtype=torch.float32, device=dev)
        self.ins, self.outs, off = [], [], 0
        for h, w in LEVELS:
            fm = C.FMap(self.xbuf, B, h, w, cin, off=off * cin, bstride=TOTAL * cin, split=split, half=dtype if split else 'bf16x3')
            fm.write(torch.randn((B, h, w, cin), generator=g))
            self.ins.append(fm)
            self.outs.append(C.FMap(self.obuf, B, h, w, cout, off=off * cout, bstride=TOTAL * cout))
            off += h * w
        k = (torch.randn((3, 3, cin, cout), generator=g) * (2.0 / (9 * cin)) ** 0.5).numpy()
        self.w = C.pack_weight(k, dtype, dev)
        self.bias = (torch.randn((cout,), generator=g) * 0.1).to(dev)
        self.scale = C.out_scale_of(k, dev) if dtype == 'f16x3' else None
        self.cin = cin
        self.rows = torch.zeros((B * TOTAL,), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((hip.GPP_MAX_GROUPS + 1,), dtype=torch.int32, device=dev)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.poison()
        C.run_conv(self.desc(0))
        self.dense = self.bits()
        assert not (self.dense == POISON).any()

    def desc(self, tile, gathered=False):
        d = C.conv_desc(self.ins, self.outs, self.w, self.bias, 3, 3, self.cin, self.cout, pad=(1, 1), dtype=self.dtype, out_f32=True,
                        tile_hint=tile, out_scale=self.scale)
        if gathered:
            d.gather_rows, d.gather_counts = self.rows.data_ptr(), self.counts.data_ptr()
        return d

    def poison(self):
        self.obuf.view(torch.int32).fill_(POISON)

    def bits(self):
        return self.obuf.view(torch.int32).cpu().numpy().copy()          # (B, TOTAL, C_out)

    def put(self, lists):
        begin = 0
        rows = np.zeros((B * TOTAL,), np.int32)
        for p, lst in zip(PIX, lists):
            rows[begin:begin + len(lst)] = lst
            begin += B * p
        self.rows.copy_(torch.as_tensor(rows))
        self.counts.copy_(torch.as_tensor([len(x) for x in lists] + [0] * (hip.GPP_MAX_GROUPS - len(lists)) + [sum(len(x) for x in lists)],
                                          dtype=torch.int32))

    def expected(self, lists):
        want = np.full_like(self.dense, POISON)
        off = 0
        for p, lst in zip(PIX, lists):
            for m in lst:
                b, q = divmod(m, p)
                want[b, off + q] = self.dense[b, off + q]
            off += p
        return want


_LAYERS = {}


def layer(dtype, split, cin, cout):
    key = (dtype, split, cin, cout)
    if key not in _LAYERS:
        _LAYERS[key] = Layer(*key)
    return _LAYERS[key]


TYPES = [('f16x3', True), ('f16x3', False), ('f32', False)] + \
        [pytest.param(t, s, marks=pytest.mark.slow) for t, s in (('bf16', False), ('f16', False), ('bf16x3', True), ('bf16x3', False))]


@pytest.mark.parametrize('cin,cout', [(64, 144), (128, 144), (64, 36), (128, 36)])
@pytest.mark.parametrize('dtype,split', TYPES)
def test_listed_rows_are_the_dense_rows_and_nothing_else_is_written(dtype, split, cin, cout):
    L = layer(dtype, split, cin, cout)
    for name, lists in pixel_lists().items():
        L.put(lists)
        want = L.expected(lists)
        for tile in [0] + tiles_of(cout):
            L.poison()
            C.run_conv(L.desc(tile, gathered=True))
            got = L.bits()
            assert np.array_equal(got, want), (name, tile, int((got != want).sum()))


def test_gathered_tiles_are_listed_and_the_scope_is_enforced():
    L = layer('f32', False, 64, 144)
    L.put(pixel_lists()['random 10 %'])
    tiles, count = (ctypes.c_int * 32)(), ctypes.c_int(0)
    d = L.desc(0, gathered=True)
    hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(d), tiles, 32, ctypes.byref(count)), 'candidates')
    assert sorted(set(tiles[:count.value]) - {0}) == sorted(GATHER_TILES)
    d36 = layer('f32', False, 64, 36).desc(0, gathered=True)
    hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(d36), tiles, 32, ctypes.byref(count)), 'candidates')
    assert sorted(set(tiles[:count.value]) - {0}) == [6032064, 6064064, 7032064, 7064064]           # 160 columns would only add padding
    dense = L.desc(0)
    hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(dense), tiles, 32, ctypes.byref(count)), 'candidates')
    assert not any(t >= 6000000 for t in tiles[:count.value])
    run = lambda desc: hip.lib().gpp_conv2d_igemm(ctypes.byref(desc), hip.stream_ptr())  # noqa: E731
    assert run(L.desc(6064064)) == -1                    # a gathered tile without a list
    assert run(L.desc(128128, gathered=True)) == -1      # a dense tile with one
    d = L.desc(0, gathered=True)
    d.split_k = 3
    assert run(d) == -4                                  # split-K would change the summation order: refused
    d = L.desc(0, gathered=True)
    d.out_f32 = 0
    assert run(d) == -4
    d = L.desc(0, gathered=True)
    d.gather_counts = None
    assert run(d) == -1


@pytest.mark.parametrize('dtype,split', [('f16x3', True), ('f32', False)])
def test_a_guarded_launch_runs_exactly_when_the_device_value_matches(dtype, split):
    L = layer(dtype, split, 64, 144)
    lists = pixel_lists()['random 10 %']
    L.put(lists)
    nothing = np.full_like(L.dense, POISON)
    for gathered, want in ((False, L.dense), (True, L.expected(lists))):
        for flag in (0, 1):
            for value in (0, 1):
                L.flag.fill_(flag)
                L.poison()
                d = L.desc(0, gathered=gathered)
                d.guard, d.guard_value = L.flag.data_ptr(), value
                C.run_conv(d)
                assert np.array_equal(L.bits(), want if flag == value else nothing), (gathered, flag, value)


# ---------------------------------------------------------------------------------------------- the list kernels against NumPy
NBA = 12                                          # base anchors per pixel (utils/anchors.NUM_BASE_ANCHORS)
N_ANCHORS = TOTAL * NBA
HEADER_BYTES, COUNTER_STRIDE = 64 * 4096, 4096    # the detect workspace (csrc/decode.hip): a counter per image, then the key lists
KEY_STRIDE = 1 << (N_ANCHORS - 1).bit_length()


def run_lists(per_image_anchors, max_rows, state=None):
    """ per_image_anchors: for every image the candidate anchors IN THE ORDER their keys stand in the workspace """
    dev = torch.device('cuda')
    if state is None:
        need = hip.c_size_t(0)
        hip.check(hip.lib().gpp_detect_workspace_bytes(B, N_ANCHORS, need), 'workspace')
        state = {'ws': torch.zeros((int(need.value),), dtype=torch.uint8, device=dev),
                 'bitmap': torch.zeros((sum((B * p + 31) // 32 for p in PIX),), dtype=torch.int32, device=dev),
                 'rows': torch.full((B * TOTAL,), -7, dtype=torch.int32, device=dev),
                 'counts': torch.full((hip.GPP_MAX_GROUPS + 1,), -7, dtype=torch.int32, device=dev),
                 'flag': torch.full((1,), -7, dtype=torch.int32, device=dev)}
    ws = np.zeros((state['ws'].numel(),), np.uint8)
    keys = ws[HEADER_BYTES:HEADER_BYTES + B * KEY_STRIDE * 8].view(np.uint64).reshape(B, KEY_STRIDE)
    for b, anchors in enumerate(per_image_anchors):
        ws[b * COUNTER_STRIDE:b * COUNTER_STRIDE + 4].view(np.int32)[0] = len(anchors)
        a = np.asarray(anchors, np.uint64)
        keys[b, :len(a)] = (np.uint64(0x3f000000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - a)
    state['ws'].copy_(torch.as_tensor(ws))
    d = hip.PixelListDesc(state['ws'].data_ptr(), state['bitmap'].data_ptr(), state['rows'].data_ptr(), state['counts'].data_ptr(),
                          state['flag'].data_ptr(), N_ANCHORS, B, NBA, 1, len(PIX), max_rows, 0, (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*PIX), 0)
    hip.check(hip.lib().gpp_detect_pixel_lists(ctypes.byref(d), hip.stream_ptr()), 'gpp_detect_pixel_lists')
    rows, counts = state['rows'].cpu().numpy(), state['counts'].cpu().numpy()
    assert not state['bitmap'].any()                                     # left empty for the next call
    lists, begin = [], 0
    for l, p in enumerate(PIX):
        lists.append(rows[begin:begin + counts[l]].tolist())
        begin += B * p
    assert counts[len(PIX):hip.GPP_MAX_GROUPS].tolist() == [0] * (hip.GPP_MAX_GROUPS - len(PIX))
    assert counts[hip.GPP_MAX_GROUPS] == sum(len(x) for x in lists)
    return lists, int(state['flag'].item()), state


def lists_np(per_image_anchors):
    first = np.concatenate([[0], np.cumsum(PIX)])
    out = [set() for _ in PIX]
    for b, anchors in enumerate(per_image_anchors):
        for a in anchors:
            pixel = int(a) // NBA
            l = int(np.searchsorted(first, pixel, side='right')) - 1
            out[l].add(b * PIX[l] + pixel - int(first[l]))
    return [sorted(s) for s in out]


def test_pixel_lists_match_numpy_whatever_the_key_order():
    rng = np.random.default_rng(3)
    state = None
    cases = {'zero candidates': [[], []],
             'all anchors': [list(range(N_ANCHORS))] * B,
             'one image only': [[], rng.choice(N_ANCHORS, size=300, replace=False).tolist()],
             'several anchors of a pixel': [[0, 1, 11, 12, 13, NBA * PIX[0], NBA * PIX[0] + 5, N_ANCHORS - 1, N_ANCHORS - NBA], [24, 25, 26]],
             'random': [rng.choice(N_ANCHORS, size=n, replace=False).tolist() for n in (517, 64)]}
    for name, anchors in cases.items():
        want = lists_np(anchors)
        total = sum(len(x) for x in want)
        got, flag, state = run_lists(anchors, total, state)
        assert got == want and flag == 0, name
        shuffled = [rng.permutation(a).tolist() for a in anchors]
        got, flag, state = run_lists(shuffled, max(total - 1, 0), state)
        assert got == want and flag == (1 if total > 0 else 0), name     # the same list from any key order; one row over the bound sets the flag
    assert lists_np(cases['all anchors']) == [list(range(B * p)) for p in PIX]


# ---------------------------------------------------------------------------------------------- plan level
def run_model(env, batch, h, w, plan_mode=None, dtype='f16x3'):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rng = np.random.default_rng(0)
        img = rng.integers(0, 256, size=(batch, h, w, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
        planes = synthetic.load_plane_database('100').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype=dtype, **({'plan': plan_mode} if plan_mode else {}))
        outs = model.predict_on_batch([img, np.tile(P_inv[None].astype(np.float32), (batch, 1, 1)), np.tile(planes[None], (batch, 1, 1))])
        plan = model.plan_for(batch, h, w, planes.shape[0], True)
        state = None
        if plan.sparse is not None:
            state = (plan.sparse.counts.cpu().numpy().copy(), int(plan.sparse.flag.item()), plan.sparse.max_rows)
        outs = outs + [plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy()]
        heads = [plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy(), plan.cls_logits.cpu().numpy()]
        names = [op[3] for op in plan.ops]
        return {'outs': outs, 'heads': heads, 'events': model.x3_range_events(), 'state': state, 'names': names,
                'ordering': plan.check_stream_ordering()}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def dense_run(batch, h, w, plan_mode=None):
    key = (batch, h, w, plan_mode)
    if key not in _RUNS:
        _RUNS[key] = run_model({'GPP_SPARSE_HEADS': '0', 'GPP_AUTOTUNE': '0'}, batch, h, w, plan_mode)
        assert _RUNS[key]['state'] is None and (_RUNS[key]['outs'][2] > 0.05).sum() > 0
    return _RUNS[key]


def same_bytes(got, want):
    assert got['ordering'] == []
    for a, b in zip(got['outs'] + got['heads'], want['outs'] + want['heads']):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert got['events'] == want['events']


@pytest.mark.parametrize('env', [{}, {'GPP_AUTOTUNE': '0'}, {'GPP_AUTOTUNE': '0', 'GPP_CLS_LANE': '0'}], ids=['tuned', 'untuned', 'default lanes'])
def test_sparse_plan_gives_the_bytes_of_the_dense_plan(env):
    """ 2 x 96 x 160: the dimension output runs gathered (the regression output is split-K at this size and stays dense) """
    got = run_model(dict(env, GPP_SPARSE_HEADS='1'), 2, 96, 160)
    counts, flag, max_rows = got['state']
    assert got['names'].count('pyramid_regression_dim') == 2 and got['names'].count('pyramid_regression_ops') == 1
    assert 0 < counts[hip.GPP_MAX_GROUPS] <= max_rows and flag == 0          # the gathered launch did the work
    same_bytes(got, dense_run(2, 96, 160))


def test_sparse_plan_with_both_outputs_gathered():
    """ 1 x 224 x 352: large enough for the split rule to leave the regression output unsplit -- both output layers run gathered """
    got = run_model({'GPP_SPARSE_HEADS': '1', 'GPP_AUTOTUNE': '0'}, 1, 224, 352)
    counts, flag, max_rows = got['state']
    assert got['names'].count('pyramid_regression_dim') == 2 and got['names'].count('pyramid_regression_ops') == 2
    assert 0 < counts[hip.GPP_MAX_GROUPS] <= max_rows and flag == 0
    same_bytes(got, dense_run(1, 224, 352))


def test_the_guard_path_gives_the_same_bytes():
    """ threshold forced to 0: every step sets the flag, the dense launches run and the gathered ones return at once """
    got = run_model({'GPP_SPARSE_HEADS': '1', 'GPP_SPARSE_HEADS_MAX_SHARE': '0', 'GPP_AUTOTUNE': '0'}, 2, 96, 160)
    counts, flag, max_rows = got['state']
    assert max_rows == 0 and counts[hip.GPP_MAX_GROUPS] > 0 and flag == 1
    same_bytes(got, dense_run(2, 96, 160))


def test_latency_plan_at_batch_1_gives_the_same_bytes():
    got = run_model({'GPP_SPARSE_HEADS': '1', 'GPP_AUTOTUNE': '0'}, 1, 96, 160, plan_mode='latency')
    assert got['state'] is not None and got['names'].count('pyramid_regression_dim') + got['names'].count('pyramid_regression_ops') >= 2
    same_bytes(got, dense_run(1, 96, 160, plan_mode='latency'))
