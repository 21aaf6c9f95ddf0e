"""
Sparse regression tower: the tower's last layer evaluated on the 3 x 3 dilation of the candidates' pixels -- the only
rows its reader, the gathered output layer, takes.

  * kernel level -- the gathered-row form of gpp_conv2d_igemm into a PRE-SPLIT map (the three-phase pipelined loop, tile codes 8xxxxxx):
    every listed row holds the bytes of the dense launch in both halves of the split map, every other byte keeps its poison, every tile
    height (and the height the device chooses) gives the same bytes, the range events are those of the listed rows, a descriptor of both
    forms (gpp_conv_desc.tower_rows) runs exactly one of them, and everything outside the form's scope is refused;
  * the dilated lists of gpp_detect_pixel_lists against a NumPy binary dilation per image and level;
  * plan level -- GPP_SPARSE_TOWER=1 against 0: the same bytes in every output and in the head tensors read whole.

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
LEVELS = [(12, 18), (6, 9), (3, 5)]
PIX = [h * w for h, w in LEVELS]
TOTAL = sum(PIX)
HEIGHTS = (128, 160, 192, 224, 256)
TILES = tuple(8000000 + bm * 1000 + 256 for bm in HEIGHTS)       # include/gpp.h: 8000000 + BM * 1000 + 256
AUTO = 8000256                                                    # the height chosen on the device
POISON = 0x7fc0dead                                               # (as a pair of halves: a NaN and a value no epilogue stores beside it)
BAD_ARG, UNSUPPORTED = -1, -4


def pixel_lists():
    """ name -> (per level the ascending list of b * H * W + p, the tiles to run it with) """
    rng = np.random.default_rng(11)
    every_tile = (0, AUTO) + TILES

    def random_share(share):
        return [sorted(rng.choice(B * p, size=max(1, int(B * p * share)), replace=False).tolist()) for p in PIX]
    lists = {'none': ([[] for _ in PIX], every_tile),
             'one pixel in a corner': ([[B * PIX[0] - 1], [], []], every_tile),
             'one pixel in the first corner': ([[0], [], []], (AUTO,)),
             'random 10 %': (random_share(0.1), every_tile),
             'random 40 %': (random_share(0.4), every_tile),
             'every pixel': ([list(range(B * p)) for p in PIX], every_tile),
             'one level empty': ([random_share(0.4)[0], [], random_share(0.4)[2]], every_tile)}
    for bm, tile in zip(HEIGHTS, TILES):          # a count one row before a tile boundary, on it, one row after it: every height
        for n in (bm - 1, bm, bm + 1):
            lists['{} rows'.format(n)] = ([sorted(rng.choice(B * PIX[0], size=n, replace=False).tolist()),
                                           sorted(rng.choice(B * PIX[1], size=7, replace=False).tolist()), [3]], (tile, AUTO))
    return lists


class Tower(object):
    """ one tower layer over the three levels: 3 x 3, pad 1, ReLU, C_in -> C_out, pre-split input and output maps; the dense result once """

    def __init__(self, dtype, cin, cout, x_scale=1.0):
        dev = torch.device('cuda')
        g = torch.Generator().manual_seed(1000 * cin + cout)
        self.dtype, self.cin, self.cout = dtype, cin, cout
        self.xbuf = torch.empty((B, TOTAL, cin), dtype=torch.float32, device=dev)
        self.obuf = torch.empty((B, TOTAL, cout), dtype=torch.float32, device=dev)
        self.fbuf = torch.empty((B, TOTAL, cout), dtype=torch.float32, device=dev)        # the same layer with a float32 output (range test)
        self.ins, self.outs, self.fouts, off = [], [], [], 0
        for h, w in LEVELS:
            fm = C.FMap(self.xbuf, B, h, w, cin, off=off * cin, bstride=TOTAL * cin, split=True, half=dtype)
            fm.write(torch.randn((B, h, w, cin), generator=g) * x_scale)
            self.ins.append(fm)
            self.outs.append(C.FMap(self.obuf, B, h, w, cout, off=off * cout, bstride=TOTAL * cout, split=True, half=dtype))
            self.fouts.append(C.FMap(self.fbuf, B, h, w, cout, off=off * cout, bstride=TOTAL * cout))
            off += h * w
        k = (torch.randn((3, 3, cin, cout), generator=g) * (2.0 / (9 * cin)) ** 0.5).numpy()
        self.w = C.pack_weight(k, dtype, dev)
        self.bias = (torch.randn((cout,), generator=g) * 0.1).to(dev)
        self.scale = C.out_scale_of(k, dev) if dtype == 'f16x3' else None
        self.rows = torch.zeros((B * TOTAL,), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((hip.GPP_MAX_GROUPS + 1,), dtype=torch.int32, device=dev)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.slot = torch.zeros((1,), dtype=torch.int64, device=dev)          # GPP_F16X3: the range counter of every launch here
        self.poison()
        C.run_conv(self.desc(0))
        self.dense = self.bits()
        assert not (self.dense == POISON).any()

    def desc(self, tile=0, form='dense', tower_tile=0, out_f32=False):
        d = C.conv_desc(self.ins, self.fouts if out_f32 else self.outs, self.w, self.bias, 3, 3, self.cin, self.cout, pad=(1, 1), relu=True,
                        dtype=self.dtype, tile_hint=tile, out_scale=self.scale, out_f32=out_f32)
        if self.dtype == 'f16x3':
            d.range_counter = self.slot.data_ptr()
        if form == 'rows':
            d.gather_rows, d.gather_counts = self.rows.data_ptr(), self.counts.data_ptr()
        elif form == 'both':
            d.tower_rows, d.tower_counts, d.tower_flag, d.tower_tile = self.rows.data_ptr(), self.counts.data_ptr(), self.flag.data_ptr(), tower_tile
        return d

    def poison(self):
        self.obuf.view(torch.int32).fill_(POISON)

    def bits(self):
        return self.obuf.view(torch.int32).cpu().numpy().copy()          # (B, TOTAL, C_out): both halves of every 32-channel block

    def put(self, lists):
        begin = 0
        rows = np.zeros((B * TOTAL,), np.int32)
        for p, lst in zip(PIX, lists):
            rows[begin:begin + len(lst)] = lst
            begin += B * p
        self.rows.copy_(torch.as_tensor(rows))
        self.counts.copy_(torch.as_tensor([len(x) for x in lists] + [0] * (hip.GPP_MAX_GROUPS - len(lists)) + [sum(len(x) for x in lists)],
                                          dtype=torch.int32))

    def listed(self, lists):
        """ (B, TOTAL) bool: the rows of the lists """
        mask = np.zeros((B, TOTAL), bool)
        off = 0
        for p, lst in zip(PIX, lists):
            for m in lst:
                b, q = divmod(m, p)
                mask[b, off + q] = True
            off += p
        return mask

    def expected(self, lists):
        return np.where(self.listed(lists)[:, :, None], self.dense, np.int32(POISON))


_LAYERS = {}


def tower(dtype, cin, cout, x_scale=1.0):
    key = (dtype, cin, cout, x_scale)
    if key not in _LAYERS:
        _LAYERS[key] = Tower(*key)
    return _LAYERS[key]


def run(desc):
    return hip.lib().gpp_conv2d_igemm(ctypes.byref(desc), hip.stream_ptr())


@pytest.mark.parametrize('cin,cout', [(256, 256), (512, 512)], ids=['one column tile', 'two column tiles'])
@pytest.mark.parametrize('dtype', ['f16x3', 'bf16x3'])
def test_listed_rows_are_the_dense_rows_in_both_halves_and_nothing_else_is_written(dtype, cin, cout):
    L = tower(dtype, cin, cout)
    for name, (lists, tiles) in pixel_lists().items():
        L.put(lists)
        want = L.expected(lists)
        for tile in tiles:
            L.poison()
            C.run_conv(L.desc(tile, form='rows'))
            got = L.bits()
            assert np.array_equal(got, want), (name, tile, int((got != want).sum()))


@pytest.mark.parametrize('dtype', ['f16x3', 'bf16x3'])
def test_the_flag_selects_exactly_one_of_the_two_forms(dtype):
    L = tower(dtype, 256, 256)
    lists = pixel_lists()['random 40 %'][0]
    L.put(lists)
    nothing = np.full_like(L.dense, POISON)
    for tower_tile in (0, AUTO, TILES[1]):
        for flag, want in ((1, L.dense), (0, L.expected(lists)), (2, nothing)):
            L.flag.fill_(flag)
            L.poison()
            C.run_conv(L.desc(0, form='both', tower_tile=tower_tile))
            assert np.array_equal(L.bits(), want), (tower_tile, flag)
    # ... whatever tile the dense half runs with
    L.flag.fill_(0)
    for dense_tile in (1256256, 128256, 3256224):
        L.poison()
        rc = run(L.desc(dense_tile, form='both'))
        assert rc in (0, UNSUPPORTED)                      # (the mixed grid refuses a layer this small)
        if rc == 0:
            assert np.array_equal(L.bits(), L.expected(lists)), dense_tile


def test_range_events_are_counted_on_the_listed_rows_only():
    """ GPP_F16X3, inputs large enough that a few activations pass the half range.  The same layer with a float32 output stores the values
    the split epilogue clamps (same K order, same epilogue arithmetic, no clamp): an event is an aligned group of 8 channels holding a
    value that the clamp changes.  The dense launch counts them all, a gathered launch those of its rows. """
    L = tower('f16x3', 256, 256, x_scale=1.2e4)
    C.run_conv(L.desc(0, out_f32=True))
    v = L.fbuf.cpu().numpy()
    events = (~(np.abs(v) <= 65504.0)).reshape(B, TOTAL, L.cout // 8, 8).any(axis=3).sum(axis=2)        # per row
    assert 0 < events.sum() < 2000 and (events > 0).sum() >= 3                   # a few, in several rows

    def count(desc):
        L.slot.zero_()
        C.run_conv(desc)
        return int(L.slot.item())
    assert count(L.desc(0)) == events.sum()
    rng = np.random.default_rng(5)
    hot = [int(m) for m in np.flatnonzero(events[:, :PIX[0]].reshape(-1) > 0)]     # level 0: row index b * PIX[0] + p
    for name, lists in (('random 40 %', pixel_lists()['random 40 %'][0]), ('none', [[], [], []]),
                        ('the rows with events in level 0', [hot, [], []]),
                        ('rows without events', [[m for m in range(B * PIX[0]) if m not in hot][:200], [], []]),
                        ('random 10 %', [sorted(rng.choice(B * p, size=B * p // 10, replace=False).tolist()) for p in PIX])):
        L.put(lists)
        want = int(events[L.listed(lists)].sum())
        for tile in (AUTO, TILES[0], TILES[4]):
            assert count(L.desc(tile, form='rows')) == want, (name, tile)
        L.flag.fill_(0)
        assert count(L.desc(0, form='both')) == want, name
    L.flag.fill_(1)
    assert count(L.desc(0, form='both')) == events.sum()


def test_the_scope_is_enforced_and_the_tiles_are_listed():
    L = tower('f16x3', 256, 256)
    L.put(pixel_lists()['random 10 %'][0])
    L.flag.fill_(0)
    tiles, count = (ctypes.c_int * 64)(), ctypes.c_int(0)

    def candidates(desc):
        hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(desc), tiles, 64, ctypes.byref(count)), 'candidates')
        return list(tiles[:count.value])
    assert sorted(candidates(L.desc(0, form='rows'))) == [0, AUTO]                 # the tuner's list: the device's own choice of height
    assert not any(t >= 6000000 for t in candidates(L.desc(0)))                    # a dense layer: no gathered tile
    assert not any(t >= 6000000 for t in candidates(L.desc(0, form='both')))       # both forms: tile_hint is the dense half's
    assert not any(t >= 8000000 for t in candidates(L.desc(0, form='rows', out_f32=True)))
    for form in ('rows', 'both'):
        def bad(**fields):
            d = L.desc(0, form=form)
            for k, val in fields.items():
                setattr(d, k, val)
            return run(d)
        assert bad() == 0
        assert bad(stride=2) == UNSUPPORTED
        assert bad(split_k=3) == UNSUPPORTED
        assert bad(C_out=128) == UNSUPPORTED                                       # whole 256-column tiles
        assert bad(x3_split=1) == UNSUPPORTED                                      # a float32-sized output map that is not pre-split
        assert bad(x3_split=2) == UNSUPPORTED                                      # ... input map
        assert bad(residual=L.obuf.data_ptr(), res_pitch=L.cout) == UNSUPPORTED   # no shortcut
        assert bad(dtype=hip.GPP_F32, x3_split=0, out_scale=None, range_counter=None) == UNSUPPORTED
        assert bad(dtype=hip.GPP_BF16, x3_split=0, out_scale=None, range_counter=None) == UNSUPPORTED
    assert run(L.desc(TILES[0])) == BAD_ARG                                        # a gathered tile without a list
    assert run(L.desc(1256256, form='rows')) == BAD_ARG                            # a dense tile with one
    assert run(L.desc(6064064, form='rows')) == UNSUPPORTED                        # the float32-output form's tile on a pre-split output
    assert run(L.desc(TILES[0], form='rows', out_f32=True)) == UNSUPPORTED         # ... and the other way round
    assert run(L.desc(8096256, form='rows')) == BAD_ARG                            # not a height of the catalogue

    def both(**fields):
        d = L.desc(0, form='both')
        for k, val in fields.items():
            setattr(d, k, val)
        return run(d)
    assert both(tower_counts=None) == BAD_ARG
    assert both(tower_flag=None) == BAD_ARG
    assert both(gather_rows=L.rows.data_ptr(), gather_counts=L.counts.data_ptr()) == BAD_ARG
    assert both(guard=L.flag.data_ptr()) == BAD_ARG
    assert both(reserved4=1) == BAD_ARG
    assert both(tower_tile=1256256) == BAD_ARG and both(tower_tile=6064064) == UNSUPPORTED
    d = L.desc(0)
    d.tower_tile = AUTO
    assert run(d) == BAD_ARG                                                       # a tower tile without the lists
    d = L.desc(0, form='both')
    d.tower_rows = L.rows.data_ptr() + 2
    assert run(d) == -3                                                            # GPP_ERR_ALIGN
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the dilated lists against NumPy
NBA = 12
N_ANCHORS = TOTAL * NBA
HEADER_BYTES, COUNTER_STRIDE = 64 * 4096, 4096    # the detect workspace (csrc/decode.hip): a counter per image, then the key lists
KEY_STRIDE = 1 << (N_ANCHORS - 1).bit_length()
FIRST = np.concatenate([[0], np.cumsum(PIX)])


def run_lists(per_image_anchors, max_rows, max_dilated, state=None):
    """ per_image_anchors: for every image the candidate anchors IN THE ORDER their keys stand in the workspace.
    Returns (lists, flag, dilated lists, dilated flag, state). """
    dev = torch.device('cuda')
    if state is None:
        need = hip.c_size_t(0)
        hip.check(hip.lib().gpp_detect_workspace_bytes(B, N_ANCHORS, need), 'workspace')
        words = sum((B * p + 31) // 32 for p in PIX)
        state = {'ws': torch.zeros((int(need.value),), dtype=torch.uint8, device=dev)}
        for k in ('', 'd_'):
            state[k + 'bitmap'] = torch.zeros((words,), dtype=torch.int32, device=dev)
            state[k + 'rows'] = torch.full((B * TOTAL,), -7, dtype=torch.int32, device=dev)
            state[k + 'counts'] = torch.full((hip.GPP_MAX_GROUPS + 1,), -7, dtype=torch.int32, device=dev)
            state[k + 'flag'] = torch.full((1,), -7, dtype=torch.int32, device=dev)
        state['d_bitmap'].fill_(-1)               # the dilated map is written whole: whatever it holds before the first call
    ws = np.zeros((state['ws'].numel(),), np.uint8)
    keys = ws[HEADER_BYTES:HEADER_BYTES + B * KEY_STRIDE * 8].view(np.uint64).reshape(B, KEY_STRIDE)
    for b, anchors in enumerate(per_image_anchors):
        ws[b * COUNTER_STRIDE:b * COUNTER_STRIDE + 4].view(np.int32)[0] = len(anchors)
        a = np.asarray(anchors, np.uint64)
        keys[b, :len(a)] = (np.uint64(0x3f000000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - a)
    state['ws'].copy_(torch.as_tensor(ws))
    d = hip.PixelListDesc(state['ws'].data_ptr(), state['bitmap'].data_ptr(), state['rows'].data_ptr(), state['counts'].data_ptr(),
                          state['flag'].data_ptr(), N_ANCHORS, B, NBA, 1, len(PIX), max_rows, 0, (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*PIX), 0)
    d.dilated_bitmap, d.dilated_rows = state['d_bitmap'].data_ptr(), state['d_rows'].data_ptr()
    d.dilated_counts, d.dilated_flag = state['d_counts'].data_ptr(), state['d_flag'].data_ptr()
    d.level_width = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*[w for _, w in LEVELS])
    d.dilated_max_rows = max_dilated
    hip.check(hip.lib().gpp_detect_pixel_lists(ctypes.byref(d), hip.stream_ptr()), 'gpp_detect_pixel_lists')
    assert not state['bitmap'].any() and not state['d_bitmap'].any()              # both maps left empty for the next call
    out = []
    for k in ('', 'd_'):
        rows, counts = state[k + 'rows'].cpu().numpy(), state[k + 'counts'].cpu().numpy()
        lists, begin = [], 0
        for l, p in enumerate(PIX):
            lists.append(rows[begin:begin + counts[l]].tolist())
            begin += B * p
        assert counts[len(PIX):hip.GPP_MAX_GROUPS].tolist() == [0] * (hip.GPP_MAX_GROUPS - len(PIX))
        assert counts[hip.GPP_MAX_GROUPS] == sum(len(x) for x in lists)
        out += [lists, int(state[k + 'flag'].item())]
    return out + [state]


def lists_np(per_image_anchors):
    """ (the lists, their 3 x 3 binary dilation per image and level) """
    masks = [np.zeros((B, h, w), bool) for h, w in LEVELS]
    for b, anchors in enumerate(per_image_anchors):
        for a in anchors:
            pixel = int(a) // NBA
            l = int(np.searchsorted(FIRST, pixel, side='right')) - 1
            masks[l][b].reshape(-1)[pixel - int(FIRST[l])] = True
    plain, dilated = [], []
    for m in masks:
        padded = np.zeros((B, m.shape[1] + 2, m.shape[2] + 2), bool)
        padded[:, 1:-1, 1:-1] = m
        grown = np.zeros_like(m)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                grown |= padded[:, dy:dy + m.shape[1], dx:dx + m.shape[2]]
        plain.append(np.flatnonzero(m.reshape(-1)).tolist())
        dilated.append(np.flatnonzero(grown.reshape(-1)).tolist())
    return plain, dilated


def anchors_of(level, pixels):
    return [int((FIRST[level] + p) * NBA + (p % NBA)) for p in pixels]


def test_dilated_lists_match_a_numpy_dilation_per_image_and_level():
    rng = np.random.default_rng(9)
    h0, w0 = LEVELS[0]
    corners = [0, w0 - 1, (h0 - 1) * w0, h0 * w0 - 1]
    borders = [y * w0 + x for y in range(h0) for x in range(w0) if y in (0, h0 - 1) or x in (0, w0 - 1)]
    cases = {'no candidate': [[], []],
             'every pixel': [list(range(0, N_ANCHORS, NBA))] * B,
             'corners of every level': [[a for l, (h, w) in enumerate(LEVELS) for a in anchors_of(l, [0, w - 1, (h - 1) * w, h * w - 1])]] * B,
             'borders of level 0': [anchors_of(0, borders), anchors_of(0, corners)],
             # the last row of image 0 and the first row of image 1, level by level: neighbours in the list, not in the picture
             'facing edges of adjacent images': [[a for l, (h, w) in enumerate(LEVELS) for a in anchors_of(l, range((h - 1) * w, h * w))],
                                                 [a for l, (h, w) in enumerate(LEVELS) for a in anchors_of(l, range(w))]],
             # the last pixel of a level and the first of the next: neighbours in the pyramid's row order only
             'facing ends of adjacent levels': [anchors_of(0, [PIX[0] - 1]) + anchors_of(1, [0]), anchors_of(1, [PIX[1] - 1]) + anchors_of(2, [0])],
             'one pixel in the middle': [anchors_of(0, [5 * w0 + 7]), []],
             'random': [rng.choice(N_ANCHORS, size=n, replace=False).tolist() for n in (300, 40)]}
    state = None
    for name, anchors in cases.items():
        plain, dilated = lists_np(anchors)
        n, nd = sum(len(x) for x in plain), sum(len(x) for x in dilated)
        got, flag, got_d, flag_d, state = run_lists(anchors, n, nd, state)
        assert got == plain and got_d == dilated and flag == 0 and flag_d == 0, name
        # the same lists from any key order, on a state the previous call left (both bitmaps cleared); one row over a bound sets that flag,
        # and the lists' own flag sets the dilated one
        shuffled = [rng.permutation(a).tolist() for a in anchors]
        got, flag, got_d, flag_d, state = run_lists(shuffled, n, max(nd - 1, 0), state)
        assert got == plain and got_d == dilated and flag == 0 and flag_d == (1 if nd > 0 else 0), name
        got, flag, got_d, flag_d, state = run_lists(shuffled, max(n - 1, 0), nd, state)
        assert got == plain and got_d == dilated and flag == flag_d == (1 if n > 0 else 0), name
    plain, dilated = lists_np(cases['one pixel in the middle'])
    assert len(plain[0]) == 1 and len(dilated[0]) == 9
    plain, dilated = lists_np(cases['facing edges of adjacent images'])
    assert len(dilated[0]) == B * 2 * w0                                          # two rows per image: nothing crossed into the other image
    # without the dilated fields the call is what it was
    d = hip.PixelListDesc(state['ws'].data_ptr(), state['bitmap'].data_ptr(), state['rows'].data_ptr(), state['counts'].data_ptr(),
                          state['flag'].data_ptr(), N_ANCHORS, B, NBA, 1, len(PIX), 5, 0, (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*PIX), 0)
    state['d_rows'].fill_(-7)
    hip.check(hip.lib().gpp_detect_pixel_lists(ctypes.byref(d), hip.stream_ptr()), 'gpp_detect_pixel_lists')
    assert (state['d_rows'] == -7).all()
    d.dilated_rows = state['d_rows'].data_ptr()
    assert hip.lib().gpp_detect_pixel_lists(ctypes.byref(d), hip.stream_ptr()) == BAD_ARG      # all four pointers or none


# ---------------------------------------------------------------------------------------------- plan level
SHAPE = (2, 224, 352)


def run_model(env):
    env = dict({'GPP_AUTOTUNE': '0', 'GPP_SPARSE_TOWER_MIN_ROUNDS': '0'}, **env)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        batch, h, w = SHAPE
        rng = np.random.default_rng(0)
        img = rng.integers(0, 256, size=(batch, h, w, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
        planes = synthetic.load_plane_database('100').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
        outs = model.predict_on_batch([img, np.tile(P_inv[None].astype(np.float32), (batch, 1, 1)), np.tile(planes[None], (batch, 1, 1))])
        plan = model.plan_for(batch, h, w, planes.shape[0], True)
        sp = plan.sparse
        state = None
        if sp is not None and sp.tower_rows is not None:
            state = (sp.tower_counts.cpu().numpy().copy(), int(sp.tower_flag.item()), sp.tower_max_rows, sp.counts.cpu().numpy().copy())
        events = model.x3_range_events()
        outs = outs + [plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy()]
        heads = [plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy(), plan.cls_logits.cpu().numpy()]
        return {'outs': outs, 'heads': heads, 'events': events, 'events_after_completion': model.x3_range_events(), 'state': state,
                'names': [op[3] for op in plan.ops], 'flops': plan.flops, 'ordering': plan.check_stream_ordering(),
                'tower': [op[3] for op in plan.ops if op[0] == 3 and op[2].tower_rows]}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def dense_tower_run():
    if 'dense' not in _RUNS:
        _RUNS['dense'] = run_model({'GPP_SPARSE_TOWER': '0'})
        assert _RUNS['dense']['state'] is None and _RUNS['dense']['tower'] == [] and (_RUNS['dense']['outs'][2] > 0.05).sum() > 0
    return _RUNS['dense']


def same_bytes(got, want):
    assert got['ordering'] == [] and got['names'] == want['names'] and got['flops'] == want['flops']
    for a, b in zip(got['outs'] + got['heads'], want['outs'] + want['heads']):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert got['events'] == got['events_after_completion']            # reading the head tensors whole counts no event a second time


def test_sparse_tower_plan_gives_the_bytes_of_the_dense_tower_plan():
    got = run_model({'GPP_SPARSE_TOWER': '1'})
    assert got['tower'] == ['pyramid_regression_3']
    counts, flag, max_rows, listed = got['state']
    total = counts[hip.GPP_MAX_GROUPS]
    assert listed[hip.GPP_MAX_GROUPS] < total <= max_rows and flag == 0          # the gathered launch did the work, on more rows than are listed
    same_bytes(got, dense_tower_run())


def test_the_dense_path_of_a_sparse_tower_plan_gives_the_same_bytes():
    """ largest share 0: every step sets the tower's flag, its dense launch runs and the gathered one returns at once """
    got = run_model({'GPP_SPARSE_TOWER': '1', 'GPP_SPARSE_TOWER_MAX_SHARE': '0'})
    counts, flag, max_rows, _ = got['state']
    assert got['tower'] == ['pyramid_regression_3'] and max_rows == 0 and counts[hip.GPP_MAX_GROUPS] > 0 and flag == 1
    same_bytes(got, dense_tower_run())


def test_the_one_round_rule_keeps_small_plans_as_they_were():
    got = run_model({'GPP_SPARSE_TOWER': '1', 'GPP_SPARSE_TOWER_MIN_ROUNDS': '1'})
    assert got['tower'] == [] and got['state'] is None
    same_bytes(got, dense_tower_run())
