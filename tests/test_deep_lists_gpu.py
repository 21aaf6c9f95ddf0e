"""
gpp_detect_deep_lists against NumPy: the marks straight from the logits are the pixel set of the keys the candidate pass
writes for the same logits (gpp_detect_stages_f32, GPP_DETECT_CANDIDATES -- the same device decision, so the sets are EQUAL, also for logits
whose scores sit on either side of the threshold in the last float32 place); the radius-2 and radius-3 lists are the 5 x 5 and 7 x 7 binary
dilations per image and level, ascending; the flags follow  f3 = (|marks| > max_rows) | (|radius 1| > tower_max_rows),
flag2 = f3 | (|radius 2| > deep_max_rows), flag1 = flag2 | (|radius 3| > deep_max_rows).

B = 3; levels of 7 x 5, 4 x 33, 2 x 3 and 1 x 1 pixels: 105 and 396 bits (no multiple of 32, levels that start on an odd word), and levels smaller
than the radius; behind them one level of 9 x 8, the only one a whole 7 x 7 window fits into.  Exact comparisons throughout: sets and integers.
"""
import ctypes

import numpy as np
import pytest
import torch

from keras_retinanet_3D.backend import hip

pytestmark = pytest.mark.gpu

B = 3
LEVELS = [(7, 5), (4, 33), (2, 3), (1, 1), (9, 8)]
PIX = [h * w for h, w in LEVELS]
TOTAL = sum(PIX)
NBA = 12
N_ANCHORS = TOTAL * NBA
FIRST = np.concatenate([[0], np.cumsum(PIX)])
WORDS = sum((B * p + 31) // 32 for p in PIX)
THR = np.float32(0.05)
GPP_DETECT_CANDIDATES = 1
HEADER_BYTES, COUNTER_STRIDE = 64 * 4096, 4096    # the detect workspace (csrc/decode.hip): a counter per image, then the key lists
KEY_STRIDE = 1 << (N_ANCHORS - 1).bit_length()
LOW, HIGH = np.float32(-9.0), np.float32(2.0)     # far below and far above the threshold
BAD_ARG = -1


class State(object):
    def __init__(self):
        dev = torch.device('cuda')
        i32 = torch.int32
        self.logits = torch.empty((B, N_ANCHORS, 8), dtype=torch.float32, device=dev)
        self.maps = [torch.full((WORDS,), -1, dtype=i32, device=dev) for _ in range(4)]      # every word is written whole, whatever it held
        self.rows = [torch.full((B * TOTAL,), -7, dtype=i32, device=dev) for _ in range(2)]
        self.counts = [torch.full((hip.GPP_MAX_GROUPS + 1,), -7, dtype=i32, device=dev) for _ in range(2)]
        self.flags = [torch.full((1,), -7, dtype=i32, device=dev) for _ in range(2)]
        self.stats = torch.full((4,), -7, dtype=i32, device=dev)
        need = hip.c_size_t(0)
        hip.check(hip.lib().gpp_detect_workspace_bytes(B, N_ANCHORS, need), 'workspace')
        self.ws = torch.zeros((int(need.value),), dtype=torch.uint8, device=dev)
        self.dummy = torch.zeros((B * N_ANCHORS * 12,), dtype=torch.float32, device=dev)
        self.det = torch.zeros((B * 128 * 12,), dtype=torch.float32, device=dev)

    def desc(self, max_rows, tower_max_rows, deep_max_rows, layer1=True):
        d = hip.DeepListDesc()
        d.cls_logits = self.logits.data_ptr()
        d.marks, d.radius1, d.radius2, d.radius3 = [m.data_ptr() for m in self.maps]
        d.rows2, d.counts2, d.flag2 = self.rows[0].data_ptr(), self.counts[0].data_ptr(), self.flags[0].data_ptr()
        if layer1:
            d.rows1, d.counts1, d.flag1 = self.rows[1].data_ptr(), self.counts[1].data_ptr(), self.flags[1].data_ptr()
        d.stats = self.stats.data_ptr()
        d.n_anchors, d.B, d.num_base_anchors, d.n_levels = N_ANCHORS, B, NBA, len(PIX)
        d.max_rows, d.tower_max_rows, d.deep_max_rows, d.score_thr = max_rows, tower_max_rows, deep_max_rows, float(THR)
        d.level_pixels = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*(PIX + [0] * (hip.GPP_MAX_GROUPS - len(PIX))))
        d.level_width = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*([w for _, w in LEVELS] + [0] * (hip.GPP_MAX_GROUPS - len(PIX))))
        return d

    def candidate_masks(self):
        """ per level (B, H, W) bool: the pixels of the keys the candidate pass writes for self.logits """
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        hip.check(hip.lib().gpp_detect_stages_f32(GPP_DETECT_CANDIDATES, p(self.logits), p(self.dummy), p(self.dummy), p(self.dummy), B, N_ANCHORS,
                                                  NBA, 1, float(THR), 0.5, 100, p(self.det), p(self.det), p(self.det), p(self.det), p(self.det),
                                                  p(self.det), p(self.det), p(self.ws), self.ws.numel(), hip.stream_ptr()), 'candidates')
        ws = self.ws.cpu().numpy()
        keys = ws[HEADER_BYTES:HEADER_BYTES + B * KEY_STRIDE * 8].view(np.uint64).reshape(B, KEY_STRIDE)
        masks = [np.zeros((B, h, w), bool) for h, w in LEVELS]
        n = 0
        for b in range(B):
            count = int(ws[b * COUNTER_STRIDE:b * COUNTER_STRIDE + 4].view(np.int32)[0])
            n += count
            for a in (np.uint64(0xFFFFFFFF) - (keys[b, :count] & np.uint64(0xFFFFFFFF))).astype(np.int64):
                pixel = int(a) // NBA
                l = int(np.searchsorted(FIRST, pixel, side='right')) - 1
                masks[l][b].reshape(-1)[pixel - int(FIRST[l])] = True
        return masks, n

    def run(self, logits, max_rows=B * TOTAL, tower_max_rows=B * TOTAL, deep_max_rows=B * TOTAL, layer1=True):
        """ -> marks as masks, [lists of radius 2, lists of radius 3], (|marks|, |radius 1|, f3), (flag2, flag1) """
        self.logits.copy_(torch.as_tensor(logits))
        d = self.desc(max_rows, tower_max_rows, deep_max_rows, layer1)
        hip.check(hip.lib().gpp_detect_deep_lists(ctypes.byref(d), hip.stream_ptr()), 'gpp_detect_deep_lists')
        words = self.maps[0].cpu().numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder='little')
        marks, begin = [], 0
        for (h, w), p in zip(LEVELS, PIX):
            n_words = (B * p + 31) // 32
            level = bits[begin * 32:(begin + n_words) * 32]
            assert not level[B * p:].any()                      # the padding of the level's last word
            marks.append(level[:B * p].astype(bool).reshape(B, h, w))
            begin += n_words
        lists = []
        for k in range(2 if layer1 else 1):
            rows, counts = self.rows[k].cpu().numpy(), self.counts[k].cpu().numpy()
            per_level, begin = [], 0
            for l, p in enumerate(PIX):
                per_level.append(rows[begin:begin + counts[l]].tolist())
                begin += B * p
            assert counts[len(PIX):hip.GPP_MAX_GROUPS].tolist() == [0] * (hip.GPP_MAX_GROUPS - len(PIX))
            assert counts[hip.GPP_MAX_GROUPS] == sum(len(x) for x in per_level)
            lists.append(per_level)
        stats = self.stats.cpu().numpy().tolist()
        flags = tuple(int(f.item()) for f in self.flags[:2 if layer1 else 1])
        assert stats[3] == flags[0]                             # flag2 as the statistics launch has it, for the radius-3 compaction beside it
        return marks, lists, tuple(stats[:3]), flags


@pytest.fixture(scope='module')
def state():
    return State()


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


def logits_of(hot, value=HIGH):
    """ hot: [(image, level, pixel, anchor of the pixel)] -> logits with one logit of each of those anchors at `value`, everything else far below """
    x = np.full((B, N_ANCHORS, 8), LOW, np.float32)
    for i, (b, l, p, k) in enumerate(hot):
        x[b, (FIRST[l] + p) * NBA + k, i % 8] = value
    return x


def masks_of(hot):
    masks = [np.zeros((B, h, w), bool) for h, w in LEVELS]
    for b, l, p, _ in hot:
        masks[l][b].reshape(-1)[p] = True
    return masks


def cases():
    rng = np.random.default_rng(3)
    h0, w0 = LEVELS[0]
    h1, w1 = LEVELS[1]
    every = [(b, l, p, (b + p) % NBA) for b in range(B) for l in range(len(PIX)) for p in range(PIX[l])]
    return {'no pixel': [],
            'every pixel': every,
            'one pixel in the middle': [(1, 4, 4 * LEVELS[4][1] + 4, 5)],
            'the four corners': [(b, l, p, 0) for b in (0, 2) for l, (h, w) in enumerate(LEVELS) for p in (0, w - 1, (h - 1) * w, h * w - 1)],
            # the last row of image 0 and the first row of image 1: neighbours in the bitmap, not in the picture
            'facing edges of adjacent images': [(0, l, p, 1) for l, (h, w) in enumerate(LEVELS) for p in range((h - 1) * w, h * w)] +
                                               [(1, l, p, 2) for l, (h, w) in enumerate(LEVELS) for p in range(w)],
            'facing ends of adjacent levels': [(2, 0, PIX[0] - 1, 0), (0, 1, 0, 0), (2, 1, PIX[1] - 1, 0), (0, 2, 0, 0), (2, 2, PIX[2] - 1, 3), (0, 3, 0, 4)],
            'several anchors of one pixel': [(1, 1, 2 * w1 + 16, k) for k in (0, 3, 11)] + [(0, 0, 0, k) for k in range(NBA)],
            'random': [(int(rng.integers(B)), l, int(rng.integers(PIX[l])), int(rng.integers(NBA))) for l in (0, 1, 1, 1, 1, 2, 4) for _ in range(4)]}


def test_marks_are_the_candidates_pixels_and_the_lists_their_dilations(state):
    for name, hot in cases().items():
        x = logits_of(hot)
        marks, lists, stats, flags = state.run(x)
        want, n_keys = state.candidate_masks()
        truth = masks_of(hot)
        assert n_keys == len(set(hot)), name
        for got, w, t in zip(marks, want, truth):
            assert np.array_equal(got, w) and np.array_equal(w, t), name
        assert lists[0] == dilate(truth, 2) and lists[1] == dilate(truth, 3), name
        n, n1 = sum(int(m.sum()) for m in truth), sum(len(v) for v in dilate(truth, 1))
        assert stats == (n, n1, 0) and flags == (0, 0), name
        # the radius-2 and radius-3 maps are compacted and cleared; the radius-1 map is the 3 x 3 dilation
        assert not state.maps[2].any() and not state.maps[3].any()
    # the sizes the section quotes: one pixel in the middle lists 25 and 49 rows; nothing crosses between images or levels
    _, lists, _, _ = state.run(logits_of(cases()['one pixel in the middle']))
    assert [len(v) for v in lists[0]] == [0, 0, 0, 0, 25] and [len(v) for v in lists[1]] == [0, 0, 0, 0, 49]
    _, lists, _, _ = state.run(logits_of([(1, 0, 3 * LEVELS[0][1] + 2, 5)]))
    assert [len(v) for v in lists[0]] == [25, 0, 0, 0, 0] and [len(v) for v in lists[1]] == [49 - 2 * 7, 0, 0, 0, 0]      # (7 x 5: the 7 x 7 window loses two columns)
    _, lists, _, _ = state.run(logits_of([(1, 1, 1 * LEVELS[1][1] + 16, 0)]))
    assert [len(v) for v in lists[0]] == [0, 4 * 5, 0, 0, 0] and [len(v) for v in lists[1]] == [0, 4 * 7, 0, 0, 0]        # (4 rows: the windows lose rows)
    _, lists, _, _ = state.run(logits_of(cases()['facing edges of adjacent images']))
    h0, w0 = LEVELS[0]
    assert len(lists[0][0]) == 2 * 3 * w0 and len(lists[1][0]) == 2 * 4 * w0           # three / four rows in each of the two images, none in the third
    assert all(m // PIX[0] in (0, 1) for m in lists[1][0])


def test_scores_next_to_the_threshold_are_decided_as_the_candidate_pass_decides_them(state):
    """ 64 consecutive float32 logits around logit(0.05), one per pixel of level 1 in every image: their scores cross the threshold in the last
    places of a float32.  Whatever the candidate pass makes of each of them, the marks make the same. """
    x0 = np.float32(np.log(0.05 / 0.95))
    values = [x0]
    for _ in range(32):
        values.append(np.nextafter(values[-1], np.float32(0)))
    lo = x0
    for _ in range(31):
        lo = np.nextafter(lo, np.float32(-10))
        values.insert(0, lo)
    assert len(values) == 64 and len(set(values)) == 64
    x = np.full((B, N_ANCHORS, 8), LOW, np.float32)
    for b in range(B):
        for i, v in enumerate(values):
            x[b, (FIRST[1] + (i * 2 + b) % PIX[1]) * NBA + (i + b) % NBA, (i + 3 * b) % 8] = v
    marks, lists, stats, _ = state.run(x)
    want, n_keys = state.candidate_masks()
    for got, w in zip(marks, want):
        assert np.array_equal(got, w)
    assert 0 < n_keys < B * 64 and stats[0] == n_keys                  # the values straddle the decision (one anchor per pixel here)
    assert lists[0] == dilate(want, 2) and lists[1] == dilate(want, 3)


def test_a_second_call_holds_nothing_of_the_first(state):
    c = cases()
    state.run(logits_of(c['every pixel']))
    for name in ('random', 'no pixel', 'the four corners'):
        truth = masks_of(c[name])
        marks, lists, _, _ = state.run(logits_of(c[name]))
        for got, t in zip(marks, truth):
            assert np.array_equal(got, t), name
        assert lists[0] == dilate(truth, 2) and lists[1] == dilate(truth, 3), name
    # layer 2 only: the radius-3 lists, counts and flag are not touched
    for t in (state.rows[1], state.counts[1], state.flags[1]):
        t.fill_(-7)
    truth = masks_of(c['random'])
    _, lists, _, flags = state.run(logits_of(c['random']), layer1=False)
    assert lists[0] == dilate(truth, 2) and flags == (0,)
    assert all(bool((t == -7).all()) for t in (state.rows[1], state.counts[1], state.flags[1]))


def test_the_flags_follow_the_chain(state):
    hot = cases()['random']
    truth = masks_of(hot)
    n, n1, n2, n3 = (sum(int(m.sum()) for m in truth),) + tuple(sum(len(v) for v in dilate(truth, r)) for r in (1, 2, 3))
    assert 0 < n < n1 < n2 < n3 < B * TOTAL
    x = logits_of(hot)
    big = B * TOTAL
    for limits, want in (((n, n1, n3), (0, 0, 0)),                    # every count exactly on its limit
                         ((n - 1, big, big), (1, 1, 1)),              # max_rows: the output layers run dense, so does everything in front
                         ((big, n1 - 1, big), (1, 1, 1)),             # tower_max_rows
                         ((n, n1, n3 - 1), (0, 0, 1)),                # deep_max_rows between the two counts: layer 1 alone
                         ((n, n1, n2), (0, 0, 1)),
                         ((n, n1, n2 - 1), (0, 1, 1)),
                         ((big, big, 0), (0, 1, 1)),                  # deep_max_rows = 0
                         ((0, big, big), (1, 1, 1)),
                         ((big, 0, big), (1, 1, 1))):
        _, lists, stats, flags = state.run(x, *limits)
        assert stats == (n, n1, want[0]) and flags == want[1:], (limits, stats, flags)
        assert lists[0] == dilate(truth, 2) and lists[1] == dilate(truth, 3)          # the lists do not depend on the limits
    # nothing marked: every count is 0 and no limit is exceeded, also at 0
    _, _, stats, flags = state.run(logits_of([]), 0, 0, 0)
    assert stats == (0, 0, 0) and flags == (0, 0)


def test_bad_descriptors_are_refused_and_handles_are_checked(state):
    lib = hip.lib()

    def rc(**fields):
        d = state.desc(1, 1, 1)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.gpp_detect_deep_lists(ctypes.byref(d), hip.stream_ptr())
    assert rc() == 0
    assert rc(marks=None) == BAD_ARG and rc(rows2=None) == BAD_ARG and rc(stats=None) == BAD_ARG and rc(cls_logits=None) == BAD_ARG
    assert rc(rows1=None) == BAD_ARG and rc(flag1=None) == BAD_ARG          # all three of layer 1 or none
    assert rc(reserved=1) == BAD_ARG and rc(deep_max_rows=-1) == BAD_ARG and rc(n_levels=0) == BAD_ARG and rc(n_anchors=N_ANCHORS + NBA) == BAD_ARG
    assert rc(level_width=(ctypes.c_int32 * hip.GPP_MAX_GROUPS)(4, 33, 3, 1, 8)) == BAD_ARG       # not a divisor of 35
    assert rc(marks=state.maps[0].data_ptr() + 2) == -3                      # GPP_ERR_ALIGN
    assert rc(B=0) == 0
    handle = ctypes.c_int32(0)
    d = state.desc(1, 1, 1)
    assert lib.gpp_detect_deep_lists_register(ctypes.byref(d), ctypes.byref(handle)) == 0 and handle.value > 0
    assert lib.gpp_detect_deep_lists_run(handle.value, 1, None) == 0
    assert lib.gpp_detect_deep_lists_release(handle.value) == 0
    assert lib.gpp_detect_deep_lists_run(handle.value, 1, None) == BAD_ARG and lib.gpp_detect_deep_lists_release(handle.value) == BAD_ARG
    assert lib.gpp_detect_deep_lists_run(0, 1, None) == BAD_ARG and lib.gpp_detect_deep_lists_run(-5, 0, None) == BAD_ARG
    torch.cuda.synchronize()
