"""
Layer 0's lists of gpp_detect_deep_lists (gpp_deep_list_desc.radius4 / rows0 / counts0 / flag0 / stats0) against a NumPy
dilation of the device's own marks: the radius-4 list is the 9 x 9 binary dilation per image and level, ascending; flag0 = flag1 |
(|radius 4| > deep_max_rows); every word of the radius-4 map is written whole over poison; and with the five fields null the call leaves in
every old output the bytes it leaves with them -- the lists of section 4.20, pinned by tests/test_deep_lists_gpu.py -- and touches nothing new.

B = 3; levels of 5 x 7, 3 x 4, 2 x 2, 1 x 1 and 1 x 1 pixels: 105, 36, 12, 3 and 3 bits, no multiple of 32, every level smaller than the 9 x 9
window in at least one direction.  Exact comparisons throughout: sets, integers and bytes.
"""
import ctypes

import numpy as np
import pytest
import torch

from keras_retinanet_3D.backend import hip

pytestmark = pytest.mark.gpu

B = 3
LEVELS = [(5, 7), (3, 4), (2, 2), (1, 1), (1, 1)]
PIX = [h * w for h, w in LEVELS]
TOTAL = sum(PIX)
NBA = 12
N_ANCHORS = TOTAL * NBA
FIRST = np.concatenate([[0], np.cumsum(PIX)])
WORDS = sum((B * p + 31) // 32 for p in PIX)
THR = np.float32(0.05)
LOW, HIGH = np.float32(-9.0), np.float32(2.0)
G = hip.GPP_MAX_GROUPS
BIG = B * TOTAL
POISON = -7
BAD_ARG, ALIGN = -1, -3
NEW = ('radius4', 'rows0', 'counts0', 'flag0', 'stats0')


class State(object):
    """ the buffers of one call: index 0 .. 3 the maps of marks and radius 1 .. 3, index 4 radius 4; lists 0, 1, 2 = layers 2, 1, 0 """

    def __init__(self):
        dev, i32 = torch.device('cuda'), torch.int32
        self.logits = torch.empty((B, N_ANCHORS, 8), dtype=torch.float32, device=dev)
        self.maps = [torch.empty((WORDS,), dtype=i32, device=dev) for _ in range(5)]
        self.rows = [torch.empty((B * TOTAL,), dtype=i32, device=dev) for _ in range(3)]
        self.counts = [torch.empty((G + 1,), dtype=i32, device=dev) for _ in range(3)]
        self.flags = [torch.empty((1,), dtype=i32, device=dev) for _ in range(3)]
        self.stats = torch.empty((5,), dtype=i32, device=dev)          # the call is handed four words; the fifth is a canary
        self.stats0 = torch.empty((2,), dtype=i32, device=dev)         # one word, and a canary
        self.poison()

    def tensors(self):
        return self.maps + self.rows + self.counts + self.flags + [self.stats, self.stats0]

    def poison(self):
        for t in self.tensors():
            t.fill_(POISON)

    def old_outputs(self):
        """ the bytes of everything section 4.20's call writes (and of the canary behind its statistics) """
        old = self.maps[:4] + self.rows[:2] + self.counts[:2] + self.flags[:2] + [self.stats]
        return [t.cpu().numpy().tobytes() for t in old]

    def desc(self, max_rows=BIG, tower_max_rows=BIG, deep_max_rows=BIG, layer0=True):
        d = hip.DeepListDesc()
        d.cls_logits = self.logits.data_ptr()
        d.marks, d.radius1, d.radius2, d.radius3 = [m.data_ptr() for m in self.maps[:4]]
        d.rows2, d.counts2, d.flag2 = self.rows[0].data_ptr(), self.counts[0].data_ptr(), self.flags[0].data_ptr()
        d.rows1, d.counts1, d.flag1 = self.rows[1].data_ptr(), self.counts[1].data_ptr(), self.flags[1].data_ptr()
        d.stats = self.stats.data_ptr()
        if layer0:
            d.radius4, d.rows0, d.counts0 = self.maps[4].data_ptr(), self.rows[2].data_ptr(), self.counts[2].data_ptr()
            d.flag0, d.stats0 = self.flags[2].data_ptr(), self.stats0.data_ptr()
        d.n_anchors, d.B, d.num_base_anchors, d.n_levels = N_ANCHORS, B, NBA, len(PIX)
        d.max_rows, d.tower_max_rows, d.deep_max_rows, d.score_thr = max_rows, tower_max_rows, deep_max_rows, float(THR)
        d.level_pixels = (ctypes.c_int32 * G)(*(PIX + [0] * (G - len(PIX))))
        d.level_width = (ctypes.c_int32 * G)(*([w for _, w in LEVELS] + [0] * (G - len(PIX))))
        return d

    def run(self, hot, layer0=True, **limits):
        """ one call over poison -> (the device's marks as masks, the lists of layers 2, 1 (and 0), the flags of layers 2, 1 (and 0)) """
        self.poison()
        self.logits.copy_(torch.as_tensor(logits_of(hot)))
        # the marks as the device makes them: read before the compactions of a second call could matter -- the marks are never cleared
        d = self.desc(layer0=layer0, **limits)
        hip.check(hip.lib().gpp_detect_deep_lists(ctypes.byref(d), hip.stream_ptr()), 'gpp_detect_deep_lists')
        bits = np.unpackbits(self.maps[0].cpu().numpy().view(np.uint8), bitorder='little')
        marks, begin = [], 0
        for (h, w), p in zip(LEVELS, PIX):
            n_words = (B * p + 31) // 32
            level = bits[begin * 32:(begin + n_words) * 32]
            assert not level[B * p:].any()
            marks.append(level[:B * p].astype(bool).reshape(B, h, w))
            begin += n_words
        lists = []
        for k in range(3 if layer0 else 2):
            rows, counts = self.rows[k].cpu().numpy(), self.counts[k].cpu().numpy()
            per_level, begin = [], 0
            for l, p in enumerate(PIX):
                per_level.append(rows[begin:begin + counts[l]].tolist())
                begin += B * p
            assert counts[len(PIX):G].tolist() == [0] * (G - len(PIX)) and counts[G] == sum(len(x) for x in per_level)
            lists.append(per_level)
        flags = tuple(int(f.item()) for f in self.flags[:3 if layer0 else 2])
        return marks, lists, flags


@pytest.fixture(scope='module')
def state():
    return State()


def logits_of(hot):
    x = np.full((B, N_ANCHORS, 8), LOW, np.float32)
    for i, (b, l, p, k) in enumerate(hot):
        x[b, (FIRST[l] + p) * NBA + k, i % 8] = HIGH
    return x


def masks_of(hot):
    masks = [np.zeros((B, h, w), bool) for h, w in LEVELS]
    for b, l, p, _ in hot:
        masks[l][b].reshape(-1)[p] = True
    return masks


def dilate(masks, r):
    """ the (2 r + 1) x (2 r + 1) binary dilation per image and level, as ascending lists b * H * W + p """
    out = []
    for m in masks:
        padded = np.zeros((B, m.shape[1] + 2 * r, m.shape[2] + 2 * r), bool)
        padded[:, r:r + m.shape[1], r:r + m.shape[2]] = m
        grown = np.zeros_like(m)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                grown |= padded[:, dy:dy + m.shape[1], dx:dx + m.shape[2]]
        out.append(np.flatnonzero(grown.reshape(-1)).tolist())
    return out


def cases():
    h0, w0 = LEVELS[0]
    return {'no pixel': [],
            'corners of two levels': [(b, l, p, b) for b in (0, 2) for l in (0, 1) for h, w in [LEVELS[l]] for p in (0, w - 1, (h - 1) * w, h * w - 1)],
            'on the borders': [(1, 0, 2 * w0, 3), (1, 0, 3 * w0 - 1, 4), (0, 0, 3, 0), (2, 0, (h0 - 1) * w0 + 3, 11), (1, 1, 4, 2)],
            'the last image only': [(2, 0, 0, 1), (2, 1, 5, 7), (2, 2, 3, 0), (2, 3, 0, 5), (2, 4, 0, 6)],
            'the first image only, one pixel': [(0, 0, 2 * w0 + 3, 9)],
            'two levels, facing ends': [(2, 0, PIX[0] - 1, 0), (0, 1, 0, 0)],
            'the two smallest levels': [(1, 3, 0, 2), (0, 4, 0, 3)]}


def test_the_radius_4_list_is_the_9_x_9_dilation_of_the_devices_marks(state):
    for name, hot in cases().items():
        marks, lists, flags = state.run(hot)
        for got, t in zip(marks, masks_of(hot)):
            assert np.array_equal(got, t), name
        want = [dilate(marks, r) for r in (2, 3, 4)]
        assert lists == want, name
        assert all(v == sorted(set(v)) for v in lists[2]), name                 # ascending, each row once
        assert flags == (0, 0, 0), name
        # every word of the radius-4 map was written over the poison, then compacted and cleared -- like the two maps in front of it
        assert not state.maps[4].any() and not state.maps[3].any() and not state.maps[2].any(), name
        assert state.stats0.cpu().numpy().tolist() == [0, POISON] and int(state.stats[4].item()) == POISON, name
    # no bleed: a pixel of the last image lists nothing in the others; the end of level 0 lists nothing in level 1 and the other way round;
    # the 5 x 7 level under a window of 9 x 9 around its centre is listed whole, the centre of a border row loses the rows outside
    _, lists, _ = state.run(cases()['the last image only'])
    assert all(m // p == 2 for v, p in zip(lists[2], PIX) for m in v) and [len(v) for v in lists[2]] == [5 * 5, 12, 4, 1, 1]
    _, lists, _ = state.run(cases()['the first image only, one pixel'])
    assert [len(v) for v in lists[2]] == [35, 0, 0, 0, 0] and lists[2][0] == list(range(35))
    _, lists, _ = state.run(cases()['two levels, facing ends'])
    assert all(m // PIX[0] == 2 for m in lists[2][0]) and all(m // PIX[1] == 0 for m in lists[2][1]) and lists[2][2:] == [[], [], []]
    _, lists, _ = state.run([(0, 0, 3, 0)])
    assert len(lists[2][0]) == 5 * 7 and len(lists[1][0]) == 4 * 7 and len(lists[0][0]) == 3 * 5
    _, lists, _ = state.run([(1, 0, 0, 0)])
    assert lists[2][0] == [35 + y * 7 + x for y in range(5) for x in range(5)]


def test_flag0_follows_flag1_and_its_own_count(state):
    hot = [(1, 0, 0, 0), (0, 1, 11, 3)]
    truth = masks_of(hot)
    n, n1, n2, n3, n4 = (sum(int(m.sum()) for m in truth),) + tuple(sum(len(v) for v in dilate(truth, r)) for r in (1, 2, 3, 4))
    assert 0 < n < n1 < n2 < n3 < n4 < BIG
    for limits, want in (((n, n1, n4), (0, 0, 0)),                       # every count on or under its limit
                         ((n, n1, n4 - 1), (0, 0, 1)),                   # flag1 at 0: flag0 by its own count
                         ((n, n1, n3), (0, 0, 1)),
                         ((n, n1, n3 - 1), (0, 1, 1)),                   # flag1 at 1 by its count: flag0 follows
                         ((n - 1, BIG, BIG), (1, 1, 1)),                 # flag1 at 1 through the chain, |radius 4| under its limit: flag0 follows
                         ((BIG, n1 - 1, BIG), (1, 1, 1)),
                         ((BIG, BIG, 0), (1, 1, 1)),
                         ((BIG, BIG, BIG), (0, 0, 0))):
        marks, lists, flags = state.run(hot, max_rows=limits[0], tower_max_rows=limits[1], deep_max_rows=limits[2])
        assert flags == want, (limits, flags)
        assert int(state.stats0[0].item()) == want[1] and int(state.stats[3].item()) == want[0]      # flag1 / flag2 as the statistics launch has them
        assert lists == [dilate(marks, r) for r in (2, 3, 4)]            # the lists do not depend on the limits
    _, _, flags = state.run([], max_rows=0, tower_max_rows=0, deep_max_rows=0)
    assert flags == (0, 0, 0)


def test_without_the_new_fields_the_old_outputs_hold_the_same_bytes_and_nothing_else_is_touched(state):
    for name, hot in cases().items():
        for limits in ({}, {'deep_max_rows': 1}, {'max_rows': 0}):
            marks, lists, flags = state.run(hot, layer0=False, **limits)
            assert lists == [dilate(marks, r) for r in (2, 3)], name
            old = state.old_outputs()
            # the buffers of layer 0 and the word behind the four statistics keep their poison
            for t in (state.maps[4], state.rows[2], state.counts[2], state.flags[2], state.stats0, state.stats[4:]):
                assert bool((t == POISON).all()), name
            marks0, lists0, flags0 = state.run(hot, layer0=True, **limits)
            assert state.old_outputs() == old, (name, limits)
            assert lists0[:2] == lists and flags0[:2] == flags


def test_the_new_fields_come_all_or_none(state):
    lib = hip.lib()

    def rc(**fields):
        d = state.desc(1, 1, 1)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.gpp_detect_deep_lists(ctypes.byref(d), hip.stream_ptr())
    assert rc() == 0
    for name in NEW:
        assert rc(**{name: None}) == BAD_ARG, name
    assert rc(**{name: None for name in NEW}) == 0
    assert rc(rows1=None, counts1=None, flag1=None) == BAD_ARG               # layer 0's lists never without layer 1's
    assert rc(radius4=state.maps[4].data_ptr() + 2) == ALIGN and rc(stats0=state.stats0.data_ptr() + 1) == ALIGN
    d = state.desc(1, 1, 1)
    d.B, d.rows0 = 0, None
    assert lib.gpp_detect_deep_lists(ctypes.byref(d), hip.stream_ptr()) == BAD_ARG      # a property of the descriptor, also at B = 0
    handle = ctypes.c_int32(0)
    d = state.desc(1, 1, 1)
    d.flag0 = None
    assert lib.gpp_detect_deep_lists_register(ctypes.byref(d), ctypes.byref(handle)) == BAD_ARG and handle.value == 0
    d = state.desc(1, 1, 1)
    assert lib.gpp_detect_deep_lists_register(ctypes.byref(d), ctypes.byref(handle)) == 0 and handle.value > 0
    assert lib.gpp_detect_deep_lists_release(handle.value) == 0
    torch.cuda.synchronize()
