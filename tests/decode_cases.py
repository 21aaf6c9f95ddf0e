"""
Constructed inputs for the selection of the decode (csrc/decode.hip: candidates_kernel, nms_kernel, emit_kernel and their
orientation_specific_filter twins), and the census that says which branch each one reaches.

The oracle (oracle/decode_np.py) selects the naive way: threshold, stable argsort, a Python greedy loop, top-k.  nms_kernel runs, per
candidate list, a bitonic sort whose barriers relax to wavefront fences under stride 128, an all-on-chip greedy NMS in which each of 1024
threads owns 8 candidate slots and the next survivor is found by ballot, above 8192 candidates a 4096-bin histogram that cuts a prefix, a
global-memory sort and a second NMS loop when that prefix is not enough, and an IoU test that evaluates the reference's division only in a
2^-19 band around the threshold.  Random logits give a few hundred keys with overlaps far from the threshold; the builders here aim at the
rest.  Every builder is deterministic, returns a Case and states, as `claims`, what the ORACLE and the census must show on it;
tests/test_decode_selection_cpu.py asserts the claims (so a builder that stops reaching its branch fails there, not silently on the
GPU), tests/test_decode_selection_gpu.py runs every case through the kernels, bit for bit against the oracle.

How the builders control a case: every logit is -9 (never a candidate at any threshold used here), then the chosen anchors are raised.
The anchor table is an input of gpp_detect_f32, so it is synthetic: a `box id` per anchor names a 10 x 10 cell of a 20-pitch grid, and the
four corner regressions are a function of the box id too, so two anchors with one box id decode to the SAME float32 box and two with
different ids to DISJOINT boxes.  That keeps the oracle's Python NMS cheap (a copy dies on its first comparison).

Nothing here imports the product path.
"""
import functools

import numpy as np

from oracle import decode_np

F = np.float32
NBA = 12                      # base anchors per pixel: n_anchors is a multiple of it (utils/anchors.NUM_BASE_ANCHORS)

# ---- constants of nms_kernel, restated (tests/test_decode_selection_cpu.py holds them against the text of csrc/decode.hip)
LDS_KEYS = 8192               # kLdsKeys: the longest list sorted and suppressed on chip
HIST_BINS = 4096              # kHistBins
BIN_ORIGIN = 0x3D000000       # float bits of 2^-5: bin = clamp((score bits - BIN_ORIGIN) >> 14, 0, 4095)
BIN_SHIFT = 14
THREADS = 1024                # kNmsThreads
OWN = LDS_KEYS // THREADS     # candidate slots per thread on chip (8)
WAVE = 64
BINS_PER_THREAD = HIST_BINS // THREADS       # the suffix scan: thread t owns bins 4t .. 4t + 3
MAX_DET_LIMIT = 128
HEADER_SLOTS = 64             # lists per call

PATHS = ('lds', 'prefix', 'prefix+fallback', 'fallback')
# The cut thread (the one thread with `above <= 8192 < above + mine`) walks its bins q = 3 .. 0 and adds each while the sum stays <= 8192.
# It cannot add all four (above + mine > 8192), so the walk ends at q = 0, 1, 2 or 3; at q = 3 none of its bins fit and the prefix is
# what the higher threads' bins hold -- which is something ('q3') or nothing at all ('q3_empty': nsel == 0, the kernel goes straight
# to the global sort).  These are the five outcomes.
OUTCOMES = ('q0', 'q1', 'q2', 'q3', 'q3_empty')

SORT_SIZES = tuple(sorted({0, 1, 2, 3} | {2 ** m + d for m in range(2, 14) for d in (-1, 0, 1)}))


def score_bin(bits):
    v = (np.asarray(bits).astype(np.int64) - BIN_ORIGIN) >> BIN_SHIFT
    return np.clip(v, 0, HIST_BINS - 1)


def position(rank, T=THREADS):
    """ where the on-chip NMS holds the candidate of sorted rank `rank`: (slot of its thread, wavefront, lane) """
    tid = rank % T
    return rank // T, tid // WAVE, tid % WAVE


def to_fused(regression, n_base=NBA):
    """ reference layout (B, A, 12) -> fused conv layout (B, P, [4A | 2A | 2A | 2A | 2A]) """
    B, n, _ = regression.shape
    r = regression.reshape(B, n // n_base, n_base, 12)
    parts = [r[..., 0:4].reshape(B, -1, 4 * n_base)] + [r[..., 4 + 2 * k:6 + 2 * k].reshape(B, -1, 2 * n_base) for k in range(4)]
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def iou_f32(a, b):
    """ the float32 overlap of two boxes (x1 y1 x2 y2) as decode_np._iou_above computes it, or None where that returns early """
    ay0, ax0, ay1, ax1 = min(a[0], a[2]), min(a[1], a[3]), max(a[0], a[2]), max(a[1], a[3])
    by0, bx0, by1, bx1 = min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])
    area_a = F(F(ay1 - ay0) * F(ax1 - ax0))
    area_b = F(F(by1 - by0) * F(bx1 - bx0))
    if area_a <= 0 or area_b <= 0:
        return None
    ih = max(F(min(ay1, by1) - max(ay0, by0)), F(0.0))
    iw = max(F(min(ax1, bx1) - max(ax0, bx0)), F(0.0))
    inter = F(ih * iw)
    return F(inter / F(F(area_a + area_b) - inter))


def iou_branch(a, b, thr):
    """ which line of iou_above_norm decides the pair at `thr`: 'sign_above', 'sign_below' (outside the guard band) or 'division' """
    ay0, ax0, ay1, ax1 = min(a[0], a[2]), min(a[1], a[3]), max(a[0], a[2]), max(a[1], a[3])
    by0, bx0, by1, bx1 = min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])
    area_a = F(F(ay1 - ay0) * F(ax1 - ax0))
    area_b = F(F(by1 - by0) * F(bx1 - bx0))
    if area_a <= 0 or area_b <= 0:
        return 'no_area'
    ih = max(F(min(ay1, by1) - max(ay0, by0)), F(0.0))
    iw = max(F(min(ax1, bx1) - max(ax0, bx0)), F(0.0))
    inter = F(ih * iw)
    uni = F(F(area_a + area_b) - inter)
    tu = F(F(thr) * uni)
    if uni > 0:
        if inter > F(tu * F(1.000002)):
            return 'sign_above'
        if inter < F(tu * F(0.999998)):
            return 'sign_below'
    return 'division'


def iou_exact(box, kept):
    """ float64 overlap of one box with each row of `kept` (the same float32 corners; every difference and product is exact in float64),
    0 where either area is not positive """
    box = np.asarray(box, np.float64)
    kept = np.asarray(kept, np.float64).reshape(-1, 4)
    lo = np.minimum(kept[:, :2], kept[:, 2:])
    hi = np.maximum(kept[:, :2], kept[:, 2:])
    blo, bhi = np.minimum(box[:2], box[2:]), np.maximum(box[:2], box[2:])
    area_k = (hi - lo).prod(axis=1)
    area_b = (bhi - blo).prod()
    inter = np.clip(np.minimum(hi, bhi) - np.maximum(lo, blo), 0.0, None).prod(axis=1)
    union = area_k + area_b - inter
    with np.errstate(all='ignore'):
        q = np.where((area_k > 0) & (area_b > 0) & (union > 0), inter / union, 0.0)
    return q


def nms_exact(boxes4, order, max_det, thr, margin):
    """ greedy NMS in float64 over candidates in `order`; returns (kept, closest): kept as indices into boxes4, and the smallest
    |overlap - thr| / thr met on the way -- a decision closer than `margin` is one float32 rounding could turn, and is an error here """
    kept, closest = [], np.inf
    for i in order:
        if len(kept) >= max_det:
            break
        if kept:
            q = iou_exact(boxes4[i], boxes4[kept])
            closest = min(closest, float(np.abs(q - thr).min()) / max(abs(thr), 1e-30))
            first = np.flatnonzero(q > thr)
            if first.size:
                continue
        kept.append(int(i))
    assert closest > margin, 'a decision within {} of the threshold: not a case for the float64 cross-check'.format(margin)
    return kept


# ---------------------------------------------------------------------------------------------------------------------------- the case

class Case(object):
    """ inputs of one call, the keyword arguments of filter_detections, and claims.  A claim is a dict with `list` = (image, orientation or
    None) and any of
        K               candidates of the list
        path            'lds' | 'prefix' | 'prefix+fallback' | 'fallback'
        outcome         where the cut thread's walk over its four bins ended (OUTCOMES)
        cut, nsel       the histogram cut and the keys above it
        kept_ranks      sorted ranks of the survivors, in order
        kept_count      their number
        last_rank_min   the last survivor's rank is at least this
        distinct        the candidates' scores are all different (True) / take exactly this many values (int)
        has, lacks      anchors among / not among the survivors
        pair_branch     ((anchor a, anchor b), branch): the line of iou_above_norm that decides the pair at the case's threshold
        bins_hit        score bins that hold a candidate
    `boundary` marks a case whose decision lies within float32 rounding of the threshold (left out of the float64 cross-check);
    `unpinned` = [(image, anchor)]: rows of these anchors are compared without box columns 6 and 10 (see case_nonfinite) """

    def __init__(self, name, logits, anchors, regression, claims=(), boundary=False, unpinned=(), pair=None, **kwargs):
        self.name = name
        self.pair = pair                                       # (anchor, anchor) of image 0 whose overlap the threshold sits at
        self.logits = np.array(logits, F, order='C')
        self.anchors = np.array(anchors, F, order='C')
        self.regression = np.array(regression, F, order='C')
        B, A = self.logits.shape[:2]
        assert A % NBA == 0 and self.anchors.shape == (A, 4) and self.regression.shape == (B, A, 12) and self.logits.shape == (B, A, 8)
        self.regression_dim = (((np.arange(B * A * 3) * 7) % 23).astype(F) / F(8.0) - F(1.0)).reshape(B, A, 3)
        self.kwargs = dict(kwargs)
        self.claims = list(claims)
        self.boundary = boundary
        self.unpinned = list(unpinned)
        self._oracle = None
        for a in (self.logits, self.anchors, self.regression, self.regression_dim):
            a.setflags(write=False)

    B = property(lambda self: self.logits.shape[0])
    A = property(lambda self: self.logits.shape[1])
    osf = property(lambda self: bool(self.kwargs.get('orientation_specific_filter', False)))
    max_det = property(lambda self: int(self.kwargs.get('max_detections', 100)))
    score_thr = property(lambda self: F(self.kwargs.get('score_threshold', 0.05)))
    # nms=False: the product passes a threshold no overlap exceeds (layers/filter_detections.py); the census models the kernel, so does the same
    iou_thr = property(lambda self: F(self.kwargs.get('nms_threshold', 0.5)) if self.kwargs.get('nms', True) else F(2.0))

    def oracle(self):
        """ ([boxes, dimensions, scores, labels, orientations], anchor indices) of oracle/decode_np.py, computed once """
        if self._oracle is None:
            with np.errstate(invalid='ignore'):                # NaN logits: the int cast inside the oracle's ldexp warns
                self._oracle = decode_np.detect(self.logits, self.regression, self.regression_dim, self.anchors, **self.kwargs)
        return self._oracle

    def tables(self):
        """ (folded scores (B, A, 4), corner boxes (B, A, 4)) as the oracle computes them """
        with np.errstate(invalid='ignore'):
            cls = decode_np.sigmoid(self.logits)
            folded = np.maximum(cls[..., :4], cls[..., 4:])
            boxes = decode_np.regress_boxes(np.broadcast_to(self.anchors[None], (self.B,) + self.anchors.shape), self.regression, cls)
        return folded, boxes[..., :4]

    def list_scores(self, folded, b, o):
        return folded[b, :, o] if o is not None else folded[b].max(axis=1)

    def lists(self):
        return [(b, o) for b in range(self.B) for o in (range(4) if self.osf else (None,))]

    def candidate_counts(self):
        """ what gpp_detect_f32 reports in `counts`: candidates per image (over the four lists with orientation_specific_filter) """
        folded, _ = self.tables()
        with np.errstate(invalid='ignore'):
            if self.osf:
                return (folded > self.score_thr).sum(axis=(1, 2)).astype(np.int32)
            return (folded.max(axis=2) > self.score_thr).sum(axis=1).astype(np.int32)


def census(case):
    """ A model of nms_kernel's control flow per candidate list, from the oracle's sigmoid bits alone: {(image, orientation): dict} with
        K, anchors (in sorted order), bits, path, cut, nsel, outcome, cut_thread, kept_ranks, kept_anchors,
        positions   (slot, wavefront, lane) of every survivor of an on-chip NMS that produced the answer ('lds', 'prefix'), else [] """
    folded, boxes = case.tables()
    ref_idx = case.oracle()[1]
    out = {}
    for b, o in case.lists():
        score = case.list_scores(folded, b, o)
        with np.errstate(invalid='ignore'):
            cand = np.flatnonzero(score > case.score_thr)
        bits = score[cand].view(np.uint32)
        key = (bits.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - cand.astype(np.uint64))
        order = np.argsort(key)[::-1]                          # keys are unique: (score desc, anchor asc)
        anchors, bits = cand[order], bits[order]
        K = int(cand.size)
        rank_of = {int(a): r for r, a in enumerate(anchors)}
        if o is None:                                          # the oracle's own answer: its NMS keeps in this same order
            kept_anchors = [int(a) for a in ref_idx[b] if a >= 0]
        elif case.kwargs.get('nms', True):
            keep = decode_np.non_max_suppression(boxes[b][cand], score[cand], case.max_det, case.iou_thr)
            kept_anchors = [int(a) for a in cand[keep]]
        else:
            kept_anchors = [int(a) for a in anchors]           # (no limit: filter_detections.py:56 skips the NMS and its max_output_size)
        kept_ranks = [rank_of[a] for a in kept_anchors]
        c = {'K': K, 'anchors': anchors, 'bits': bits, 'kept_anchors': kept_anchors, 'kept_ranks': kept_ranks,
             'cut': None, 'nsel': None, 'outcome': None, 'cut_thread': None}
        if K <= LDS_KEYS:
            c['path'], on_chip = 'lds', K
        else:
            hist = np.bincount(score_bin(bits), minlength=HIST_BINS)
            own = hist.reshape(THREADS, BINS_PER_THREAD)
            mine = own.sum(axis=1)
            above = np.concatenate([np.cumsum(mine[::-1])[::-1][1:], [0]])
            t = np.flatnonzero((above <= LDS_KEYS) & (above + mine > LDS_KEYS))
            assert t.size == 1
            t = int(t[0])
            acc, cut, stop = int(above[t]), BINS_PER_THREAD * t + BINS_PER_THREAD, None
            for q in range(BINS_PER_THREAD - 1, -1, -1):
                if acc + own[t, q] <= LDS_KEYS:
                    acc += int(own[t, q])
                    cut = BINS_PER_THREAD * t + q
                else:
                    stop = q
                    break
            assert stop is not None
            c['cut'], c['nsel'], c['cut_thread'] = cut, acc, t
            c['outcome'] = 'q3_empty' if (stop == 3 and acc == 0) else 'q{}'.format(stop)
            assert acc == int((score_bin(bits) >= cut).sum()) and (acc == 0 or np.all(score_bin(bits[:acc]) >= cut))
            # the kernel's NMS loop stops at max_det, nms or not
            reach = kept_ranks[:case.max_det]
            if acc == 0:
                c['path'] = 'fallback'
            elif len(reach) >= case.max_det and max(reach) < acc:
                c['path'] = 'prefix'
            else:
                c['path'] = 'prefix+fallback'
            on_chip = acc if c['path'] == 'prefix' else 0
        c['positions'] = [position(r) for r in kept_ranks[:case.max_det]] if on_chip else []
        out[(b, o)] = c
    return out


def failed_claims(case, cen):
    """ the claims of a case that oracle and census do not bear out, as readable strings (empty = all hold) """
    bad = []
    _, boxes = case.tables()
    for claim in case.claims:
        c = cen[claim['list']]
        b = claim['list'][0]
        checks = {
            'K': lambda v: c['K'] == v,
            'path': lambda v: c['path'] == v,
            'outcome': lambda v: c['outcome'] == v,
            'cut': lambda v: c['cut'] == v,
            'nsel': lambda v: c['nsel'] == v,
            'kept_ranks': lambda v: c['kept_ranks'][:case.max_det] == list(v),
            'kept_count': lambda v: len(c['kept_ranks'][:case.max_det]) == v,
            'last_rank_min': lambda v: c['kept_ranks'][:case.max_det][-1] >= v,
            'distinct': lambda v: np.unique(c['bits']).size == (c['K'] if v is True else v),
            'has': lambda v: set(v) <= set(c['kept_anchors'][:case.max_det]),
            'lacks': lambda v: not (set(v) & set(c['kept_anchors'][:case.max_det])),
            'pair_branch': lambda v: iou_branch(boxes[b, v[0][0]], boxes[b, v[0][1]], case.iou_thr) == v[1],
            'bins_hit': lambda v: set(v) <= set(score_bin(c['bits']).tolist()),
        }
        for k, v in claim.items():
            if k != 'list' and not checks[k](v):
                bad.append('{} list {}: {} = {!r} does not hold (K {}, path {}, outcome {}, cut {}, nsel {}, kept {} ...)'.format(
                    case.name, claim['list'], k, v, c['K'], c['path'], c['outcome'], c['cut'], c['nsel'], c['kept_ranks'][:8]))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------- inputs

GRID_W = 128


def cells(ids):
    """ anchors (n, 4) of box ids: the 10 x 10 cell of a 20-pitch grid, 128 cells to a row (every coordinate exact in float32) """
    ids = np.asarray(ids, np.int64)
    x, y = 20.0 * (ids % GRID_W), 20.0 * (ids // GRID_W)
    return np.stack([x, y, x + 10.0, y + 10.0], axis=1).astype(F)


def corner_deltas(ids):
    """ the four corner regressions of box ids, in [-0.2, 0.2]: the decoded corners move by under half a pixel, the cells stay disjoint,
    and equal ids still decode to equal boxes """
    ids = np.asarray(ids, np.int64)
    return (((ids[:, None] * 7 + np.arange(4)[None] * 3) % 11 - 5) / 25.0).astype(F)


def inputs(B, box_ids):
    """ logits at -9, the anchors and regressions of `box_ids` (A,), regressions 4..11 a pattern that is never read by the selection """
    box_ids = np.asarray(box_ids, np.int64)
    A = box_ids.size
    logits = np.full((B, A, 8), -9.0, F)
    reg = np.empty((B, A, 12), F)
    reg[:, :, :4] = corner_deltas(box_ids)[None]
    reg[:, :, 4:] = (((np.arange(B * A * 8) * 5) % 19).astype(F) / F(6.0) - F(1.5)).reshape(B, A, 8)
    return logits, cells(box_ids), reg


def pad12(n):
    return -(-n // NBA) * NBA


def rank_logits(K, hi=5.0, lo=-2.5):
    """ K logits, descending, whose sigmoids are all different and above 0.05 """
    return np.linspace(hi, lo, max(K, 1)).astype(F)[:K]


def raise_anchors(logits, b, anchors, values, channel=None):
    """ the chosen anchors become candidates: one logit each, in a channel that walks over the eight (orientation and sign vary) """
    anchors = np.asarray(anchors, np.int64)
    logits[b, anchors, anchors % 8 if channel is None else channel] = values


@functools.lru_cache(maxsize=None)
def bin_logits():
    """ {score bin: a logit whose oracle sigmoid falls into it}, from a fine grid of logits """
    grid = np.arange(-3.6, 9.0, 2e-5).astype(F)
    bins = score_bin(decode_np.sigmoid(grid).view(np.uint32))
    uniq, idx, counts = np.unique(bins, return_index=True, return_counts=True)      # the sigmoid is monotone here: a bin is one run of the grid
    return {int(u): grid[i + n // 2] for u, i, n in zip(uniq, idx, counts)}


def logit_in_bin(b):
    return bin_logits()[int(b)]


# ---- sort sizes

def case_sort(name, Ks, seed, values=None, **kwargs):
    """ one image per K: K candidates at shuffled anchors with pairwise disjoint boxes, so the answer is the top max_det of the sort.
    values None: all scores different; else the logits are drawn from `values` and the anchor half of the key decides most of the order """
    rng = np.random.default_rng(seed)
    A = pad12(max(Ks))
    logits, anchors, reg = inputs(len(Ks), np.arange(A))
    claims = []
    for b, K in enumerate(Ks):
        chosen = rng.permutation(A)[:K]
        v = rng.permutation(rank_logits(K)) if values is None else rng.choice(np.asarray(values, F), size=K)
        raise_anchors(logits, b, chosen, v)
        claim = {'list': (b, None), 'K': K, 'kept_ranks': range(min(K, int(kwargs.get('max_detections', 100))))}
        if K <= LDS_KEYS:
            claim['path'] = 'lds'
        if values is None:
            claim['distinct'] = True
        elif K >= 64:
            claim['distinct'] = len(values)
        claims.append(claim)
    return Case(name, logits, anchors, reg, claims=claims, **kwargs)


EXTRA_SIZES = (6, 11, 24, 48, 100, 101, 127, 200, 300, 500, 700, 1000, 1500, 2000, 2500, 3000, 3500, 4000, 5000, 6000, 7000, 8000, 8100, 8190, 8200)
TIE_SIZES = SORT_SIZES + EXTRA_SIZES                          # 39 + 25 = 64 images: the header-slot limit


# ---- ownership and ballots

OWNERSHIP_RANKS = tuple(sorted(({q * THREADS + w * WAVE + l for q in range(OWN) for w in (0, 7, 15) for l in (0, 63)} |
                                {1, 1023, 1024, 1025, 8191}) - {0}))


def case_ownership():
    """ K = 8192, the LDS full: every candidate is a copy of the best-scoring candidate's box except the survivor set S, mutually disjoint,
    at the sorted ranks OWNERSHIP_RANKS: every slot 0..7 of a thread, wavefronts 0, 7, 15, lanes 0 and 63, and the ranks around the
    slot boundary.  The answer: rank 0, then S in rank order.  Anchors are shuffled against ranks """
    K = LDS_KEYS
    A = pad12(K)
    rng = np.random.default_rng(77)
    anchor_of_rank = rng.permutation(A)[:K]
    ids = np.zeros(A, np.int64)
    ids[anchor_of_rank[list(OWNERSHIP_RANKS)]] = 1 + np.arange(len(OWNERSHIP_RANKS))
    logits, anchors, reg = inputs(1, ids)
    raise_anchors(logits, 0, anchor_of_rank, rank_logits(K, hi=5.5))
    claims = [{'list': (0, None), 'K': K, 'path': 'lds', 'distinct': True, 'kept_ranks': (0,) + OWNERSHIP_RANKS}]
    return Case('ownership', logits, anchors, reg, claims=claims)


# ---- clusters

CLUSTER_MEMBERS = 3
CLUSTER_STRIDE = 132          # anchor m * 132 + c is member m of cluster c (up to 129 clusters)


def cluster_counts(max_det):
    return sorted({c for c in (1, 2, max_det - 1, max_det, max_det + 1) if c >= 1})


def case_clusters(max_det):
    """ C clusters of three identical boxes, ranks interleaved (rank m * C + c is member m of cluster c): the second and third member of
    cluster c are suppressed by the box kept c-th, not by the first.  One image per C """
    Cs = cluster_counts(max_det)
    A = CLUSTER_MEMBERS * CLUSTER_STRIDE
    ids = np.arange(A) % CLUSTER_STRIDE
    logits, anchors, reg = inputs(len(Cs), ids)
    claims = []
    for b, C in enumerate(Cs):
        rank = np.arange(CLUSTER_MEMBERS * C)
        raise_anchors(logits, b, (rank // C) * CLUSTER_STRIDE + rank % C, rank_logits(rank.size))
        claims.append({'list': (b, None), 'K': CLUSTER_MEMBERS * C, 'path': 'lds', 'distinct': True, 'kept_ranks': range(min(C, max_det))})
    return Case('clusters_max_det_{}'.format(max_det), logits, anchors, reg, claims=claims, max_detections=max_det)


# ---- the threshold boundary

PAIR_OVERLAPS = (0.05, 0.15, 0.3, 0.45, 0.55, 0.7, 0.85, 0.95)
PAIR_ORIGINS = (1.0, 40.0, 100.0, 200.0, 400.0, 800.0, 1300.0, 2000.0)
THRESHOLDS = ('below', 'at', 'above', 'band_below', 'band_above')


def pair_anchors(p):
    """ two anchors whose boxes overlap by about PAIR_OVERLAPS[p], at coordinates of magnitude PAIR_ORIGINS[p], sides no round numbers """
    t, o = PAIR_OVERLAPS[p], PAIR_ORIGINS[p]
    w, h = 7.3 + 2.1 * p, 5.1 + 1.7 * p
    s = (1.0 - t) / (1.0 + t) * w * 1.0746                    # (a zero regression decodes to a box 0.0373 of the width wider on either side)
    return np.array([[o, o * 0.77 + 0.3, o + w, o * 0.77 + 0.3 + h], [o + s, o * 0.77 + 0.3, o + s + w, o * 0.77 + 0.3 + h]], F)


def pair_threshold(q, which):
    q = F(q)
    return {'below': np.nextafter(q, F(0)), 'at': q, 'above': np.nextafter(q, F(1)),
            'band_below': F(np.float64(q) * (1 - 3e-6)), 'band_above': F(np.float64(q) * (1 + 3e-6))}[which]


def pair_claims(li, first, second, which):
    """ the comparison is strict: at the overlap itself and above it the second box survives """
    suppressed = which in ('below', 'band_below')
    branch = {'below': 'division', 'at': 'division', 'above': 'division', 'band_below': 'sign_above', 'band_above': 'sign_below'}[which]
    return {'list': li, 'has': [first] + ([] if suppressed else [second]), 'lacks': [second] if suppressed else [],
            'pair_branch': ((first, second), branch)}


def pair_regression(B, A):
    reg = np.zeros((B, A, 12), F)
    reg[:, :, 4:] = (((np.arange(B * A * 8) * 5) % 19).astype(F) / F(6.0) - F(1.5)).reshape(B, A, 8)
    return reg


def decoded(anchors, reg):
    logits = np.full(reg.shape[:2] + (8,), -9.0, F)
    return decode_np.regress_boxes(anchors[None], reg[:1], decode_np.sigmoid(logits[:1]))[0, :, :4]


def case_pair_lds(p, which):
    """ eight pairs on chip (anchors 2p, 2p + 1, the first with the higher score); the threshold sits at pair p's float32 overlap,
    one ulp to either side, and just outside the guard band on either side """
    A = 24
    anchors = np.zeros((A, 4), F)
    for k in range(8):
        anchors[2 * k:2 * k + 2] = pair_anchors(k)
    anchors[16:] = cells(np.arange(8) + 40 * GRID_W)            # (unused anchors, out of the way)
    reg = pair_regression(1, A)
    logits = np.full((1, A, 8), -9.0, F)
    raise_anchors(logits, 0, np.arange(16), rank_logits(16, hi=3.0, lo=0.0))
    box = decoded(anchors, reg)
    q = iou_f32(box[2 * p], box[2 * p + 1])
    assert abs(float(q) - PAIR_OVERLAPS[p]) < 0.02
    thr = pair_threshold(q, which)
    claims = [dict(pair_claims((0, None), 2 * p, 2 * p + 1, which), K=16, path='lds')]
    return Case('pair_lds_{}_{}'.format(p, which), logits, anchors, reg, claims=claims, boundary=True, pair=(2 * p, 2 * p + 1),
                nms_threshold=float(thr))


GLOBAL_PAIRS = (1, 4, 6)      # of PAIR_OVERLAPS / PAIR_ORIGINS: overlaps 0.15, 0.55, 0.85
GLOBAL_K = 8200


def case_pair_global(g, which):
    """ the same on the global-memory path (greedy_nms, iou_above): 8200 candidates.  Pairs 0 and 1 with every score equal, so one bin
    overflows the LDS, nsel == 0, and the tie puts the candidates in anchor order; pair 2 under a top bin of ten copies of the filler,
    whose prefix yields one box.  The filler box (anchor 0 and all copies) is kept first and suppresses its copies at once; the three
    pairs sit at the last six ranks """
    A = pad12(GLOBAL_K)
    anchors = np.repeat(cells([50 * GRID_W]), A, axis=0)
    for k, p in enumerate(GLOBAL_PAIRS):
        anchors[GLOBAL_K - 6 + 2 * k:GLOBAL_K - 4 + 2 * k] = pair_anchors(p)
    reg = pair_regression(1, A)
    logits = np.full((1, A, 8), -9.0, F)
    raise_anchors(logits, 0, np.arange(GLOBAL_K), F(1.25))
    first = GLOBAL_K - 6 + 2 * g
    claim = pair_claims((0, None), first, first + 1, which)
    del claim['pair_branch']                                   # greedy_nms always divides
    if g == 2:
        raise_anchors(logits, 0, np.arange(10), F(2.0))
        claim.update(path='prefix+fallback', nsel=10)
    else:
        claim.update(path='fallback', nsel=0)
    box = decoded(anchors, reg)
    thr = pair_threshold(iou_f32(box[first], box[first + 1]), which)
    claim.update(K=GLOBAL_K, has=[0] + claim['has'])
    return Case('pair_global_{}_{}'.format(g, which), logits, anchors, reg, claims=[claim], boundary=True, pair=(first, first + 1),
                nms_threshold=float(thr))


def case_identical(which):
    """ two identical boxes overlap by exactly 1.0: at threshold 1.0 nothing is suppressed (strict), one ulp below the copy is """
    logits, anchors, reg = inputs(1, [3, 3, 5, 5, 5, 9, 0, 0, 0, 0, 0, 0])
    raise_anchors(logits, 0, np.arange(6), rank_logits(6, hi=2.0, lo=0.0))
    thr = F(1.0) if which == 'one' else np.nextafter(F(1.0), F(0))
    kept = [0, 1, 2, 3, 4, 5] if which == 'one' else [0, 2, 5]
    claims = [{'list': (0, None), 'K': 6, 'path': 'lds', 'kept_ranks': kept, 'pair_branch': ((0, 1), 'division')}]
    return Case('identical_thr_{}'.format(which), logits, anchors, reg, claims=claims, boundary=True, nms_threshold=float(thr))


def case_zero_area():
    """ an anchor of width 0 decodes to a box of area 0: it neither suppresses (rank 0, inside the box of rank 1, and its own copy at
    rank 2) nor is suppressed (rank 2; rank 4, a zero-area box inside the kept box of rank 1).  Rank 3 is a copy of rank 1 and goes """
    logits, anchors, reg = inputs(1, [3] * NBA)
    anchors = anchors.copy()
    anchors[[0, 2, 4], 2] = anchors[[0, 2, 4], 0]              # x2 = x1: w = 0, every x of the box collapses to x1
    raise_anchors(logits, 0, np.arange(5), rank_logits(5, hi=2.0, lo=0.0))
    claims = [{'list': (0, None), 'K': 5, 'kept_ranks': [0, 1, 2, 4], 'pair_branch': ((0, 1), 'no_area')}]
    return Case('zero_area', logits, anchors, reg, claims=claims)


def case_inverted():
    """ a large negative regression of x2 puts it left of x1 (99.6 -> 71.2): the overlap test sorts the corners.  Anchor 1, inside the
    sorted box and 0.70 of its area, is suppressed; anchor 2, inside the box as the unsorted corners would give it, is not """
    A = NBA
    anchors = np.repeat(cells([60 * GRID_W]), A, axis=0)
    anchors[0] = (100.0, 100.0, 110.0, 110.0)
    anchors[1] = (75.0, 100.0, 95.0, 110.0)
    anchors[2] = (100.0, 100.0, 110.0, 110.0)
    reg = pair_regression(1, A)
    reg[0, 0, 2] = -20.0
    logits = np.full((1, A, 8), -9.0, F)
    raise_anchors(logits, 0, np.arange(3), rank_logits(3, hi=2.0, lo=0.0))
    box = decoded(anchors, reg)
    assert box[0, 2] < box[0, 0] and 0.6 < iou_f32(box[0], box[1]) < 0.8 and iou_f32(box[0], box[2]) == 0
    return Case('inverted_corners', logits, anchors, reg, claims=[{'list': (0, None), 'K': 3, 'kept_ranks': [0, 2]}])


def case_no_nms():
    """ nms=False: threshold and top-k only, over clusters of copies that an NMS would thin out """
    logits, anchors, reg = inputs(2, np.arange(240) % 7)
    raise_anchors(logits, 0, np.arange(0, 240, 2), np.random.default_rng(3).permutation(rank_logits(120)))
    raise_anchors(logits, 1, np.arange(60), rank_logits(60))
    claims = [{'list': (0, None), 'K': 120, 'kept_ranks': range(100)}, {'list': (1, None), 'K': 60, 'kept_ranks': range(60)}]
    return Case('no_nms', logits, anchors, reg, claims=claims, nms=False)


# ---- pre-selection (K > 8192)

def case_binned(name, groups, claim, seed=5, **kwargs):
    """ one image from `groups`, best score first: (logit or array of logits, keys, distinct boxes).  A group's first `distinct` keys
    (by anchor) get boxes of their own, the others are copies of the image's first box.  Anchors are shuffled against groups; inside
    a group of equal scores the anchor index orders the keys """
    rng = np.random.default_rng(seed)
    K = sum(n for _, n, _ in groups)
    A = pad12(K + 17)
    chosen = rng.permutation(A)[:K]
    ids = np.zeros(A, np.int64)
    logits_of, at, next_id = np.empty(K, F), 0, 1
    for value, n, distinct in groups:
        members = np.sort(chosen[at:at + n])
        chosen[at:at + n] = members
        logits_of[at:at + n] = value
        first = 1 if at == 0 else 0                            # (the image's first box is box id 0 itself)
        ids[members[first:distinct]] = next_id + np.arange(max(distinct - first, 0))
        next_id += max(distinct - first, 0)
        at += n
    logits, anchors, reg = inputs(1, ids)
    raise_anchors(logits, 0, chosen, logits_of)
    return Case(name, logits, anchors, reg, claims=[dict({'list': (0, None), 'K': K}, **claim)], **kwargs)


PRE_BIN = 2306                # 4 * 576 + 2: a bin of the binade [0.5, 1), scores about 0.75


def pre_cases():
    lb = logit_in_bin
    T = PRE_BIN // 4
    b3, b2, b1 = 4 * T + 3, 4 * T + 2, 4 * T + 1
    cases = {}
    # the bins above the cut hold exactly 8192 keys: the LDS full, the walk ends at the third bin
    cases['pre_exactly_8192'] = functools.partial(
        case_binned, 'pre_exactly_8192', [(lb(b3), 4000, 150), (lb(b2), 4192, 30), (lb(b1), 200, 30)],
        {'path': 'prefix', 'outcome': 'q1', 'cut': b2, 'nsel': 8192, 'kept_count': 100})
    # one key more: the boundary bin is left out
    cases['pre_8193'] = functools.partial(
        case_binned, 'pre_8193', [(lb(b3), 4000, 150), (lb(b2), 4193, 30), (lb(b1), 200, 30)],
        {'path': 'prefix', 'outcome': 'q2', 'cut': b3, 'nsel': 4000, 'kept_count': 100})
    # a top bin alone overflows, all scores equal: nsel == 0, straight to the global sort, ties by anchor
    cases['pre_top_bin_overflows'] = functools.partial(
        case_binned, 'pre_top_bin_overflows', [(lb(b3), 8300, 150)],
        {'path': 'fallback', 'outcome': 'q3_empty', 'cut': b3 + 1, 'nsel': 0, 'kept_count': 100, 'distinct': 1})
    # a small top bin over one that overflows: the prefix gives 50 boxes, then the fallback
    small_top = [(lb(b3), 50, 50), (lb(b2), 8200, 200)]
    cases['pre_small_top_fallback'] = functools.partial(
        case_binned, 'pre_small_top_fallback', small_top,
        {'path': 'prefix+fallback', 'outcome': 'q2', 'cut': b3, 'nsel': 50, 'kept_count': 100, 'last_rank_min': 50})
    # the same inputs, max_det small enough for the prefix
    cases['pre_small_top_enough'] = functools.partial(
        case_binned, 'pre_small_top_enough', small_top,
        {'path': 'prefix', 'outcome': 'q2', 'cut': b3, 'nsel': 50, 'kept_count': 40}, max_detections=40)
    # the prefix yields exactly max_det boxes / one fewer, so that the last box of the answer scores below the cut
    cases['pre_prefix_exactly_max_det'] = functools.partial(
        case_binned, 'pre_prefix_exactly_max_det', [(lb(b3), 300, 100), (lb(b2), 8200, 50)],
        {'path': 'prefix', 'outcome': 'q2', 'nsel': 300, 'kept_count': 100})
    cases['pre_prefix_one_short'] = functools.partial(
        case_binned, 'pre_prefix_one_short', [(lb(b3), 300, 99), (lb(b2), 8200, 50)],
        {'path': 'prefix+fallback', 'outcome': 'q2', 'nsel': 300, 'kept_count': 100, 'last_rank_min': 300})
    # score_threshold 0.01 and 8000 scores under 2^-5: their bins are negative and clamp to 0; the walk ends at the thread's last bin
    low = np.linspace(-3.5, -4.5, 8000).astype(F)
    cases['pre_bin0_clamps'] = functools.partial(
        case_binned, 'pre_bin0_clamps', [(lb(40), 250, 30), (lb(3), 20, 10), (lb(2), 20, 10), (lb(1), 20, 10), (low, 8000, 60)],
        {'path': 'prefix+fallback', 'outcome': 'q0', 'cut': 1, 'nsel': 310, 'kept_count': 100, 'last_rank_min': 310, 'bins_hit': [0, 1, 2, 3]},
        score_threshold=0.01)
    # scores of exactly 1.0 (logit >= 17) are bin 2560; the bin under it overflows: none of the cut thread's bins fit
    cases['pre_score_one'] = functools.partial(
        case_binned, 'pre_score_one', [(F(17.5), 150, 120), (F(7.5), 8850, 30)],
        {'path': 'prefix', 'outcome': 'q3', 'cut': 2560, 'nsel': 150, 'kept_count': 100, 'bins_hit': [2559, 2560]})
    return cases


# ---- non-finite logits

NAN = F(np.nan)


def nonfinite_logits():
    """ (2, 24, 8): image 0 anchor by anchor, image 1 NaN throughout """
    logits = np.full((2, 24, 8), -9.0, F)
    l0 = logits[0]
    l0[0, 2] = np.inf                     # score 1.0
    l0[1, 3] = -np.inf                    # never a candidate
    l0[2, 1], l0[2, 5] = NAN, 2.0         # a NaN next to a passing logit of the same orientation
    l0[3, 6] = NAN                        # a NaN next to logits at -9
    l0[4, :] = NAN                        # all eight
    l0[5, 0], l0[5, 1], l0[5, 6] = NAN, 1.5, 1.0     # orientation 0 NaN; orientations 1 and 2 finite and passing
    l0[6, 4], l0[6, 3] = NAN, -np.inf     # orientation 0 NaN, nothing passes
    for a in range(7, 12):                # ordinary candidates around them
        l0[a, a % 8] = 0.25 * a - 2.0
    l0[12, 7], l0[12, 0] = np.inf, 3.0    # +inf beside a finite passing logit
    logits[1] = NAN
    return logits


def case_nonfinite(osf):
    """ The oracle's fold propagates NaN (np.maximum, then `NaN > threshold` is false): an anchor with a NaN among its logits is no
    candidate; with orientation_specific_filter it enters the lists of the orientations whose two logits are both finite.  There, box
    columns 6 and 10 of such an anchor's rows carry a sign that RegressBoxes takes from an argmax over scores with a NaN among them --
    no golden pins what that gives, so those two columns of those rows are left out of the comparison (`unpinned`); everything else of
    the rows is compared """
    logits = nonfinite_logits()
    _, anchors, reg = inputs(2, np.arange(24))
    if not osf:
        claims = [{'list': (0, None), 'K': 7, 'has': [0, 12, 7, 11], 'lacks': [1, 2, 3, 4, 5, 6]}, {'list': (1, None), 'K': 0}]
        return Case('nonfinite', logits, anchors, reg, claims=claims)
    claims = [{'list': (0, 0), 'lacks': [2, 4, 5, 6], 'has': [12]}, {'list': (0, 1), 'has': [5], 'lacks': [2, 4]}, {'list': (0, 2), 'has': [0, 5], 'lacks': [3, 4]},
              {'list': (0, 3), 'lacks': [4]}] + [{'list': (1, o), 'K': 0} for o in range(4)]
    return Case('nonfinite_osf', logits, anchors, reg, claims=claims, unpinned=[(0, 5)], orientation_specific_filter=True)


# ---- four full lists

def case_four_full_lists():
    """ orientation_specific_filter, max_det 128, 144 disjoint boxes that all pass in every orientation with the SAME score in all four:
    each list keeps 128, emit_osf_kernel's block of 512 is full, and between equal scores the earlier position (the lower orientation,
    then the better rank) comes first.  Three score values only, so most of the order is ties """
    A = 144
    logits, anchors, reg = inputs(1, np.arange(A))
    v = np.random.default_rng(11).choice(np.array([0.5, 1.0, 1.5], F), size=A)
    for o in range(4):
        logits[0, :, o + 4 * (o % 2)] = v
    claims = [{'list': (0, o), 'K': A, 'kept_count': 128, 'distinct': 3} for o in range(4)]
    return Case('four_full_lists', logits, anchors, reg, claims=claims, orientation_specific_filter=True, max_detections=128)


# ---- workspace reuse

def workspace_sequence():
    """ four calls for ONE FilterDetections instance (same batch, anchors and thresholds): a fallback case, which leaves 8300 sorted keys,
    their zero padding up to 16384, alive bytes and 100 kept-key slots behind; an lds case of 3000 candidates; an empty image; the
    first again """
    first = get('pre_top_bin_overflows')
    A = first.A
    rng = np.random.default_rng(19)
    logits = np.full((1, A, 8), -9.0, F)
    raise_anchors(logits, 0, rng.permutation(A)[:3000], rng.permutation(rank_logits(3000)))
    second = Case('reuse_lds', logits, first.anchors, first.regression, claims=[{'list': (0, None), 'K': 3000, 'path': 'lds'}])
    third = Case('reuse_empty', np.full((1, A, 8), -9.0, F), first.anchors, first.regression, claims=[{'list': (0, None), 'K': 0, 'path': 'lds'}])
    return [first, second, third, first]


BUILDERS = {}
BUILDERS['sort_distinct'] = functools.partial(case_sort, 'sort_distinct', SORT_SIZES, 1)
BUILDERS['sort_ties_b64'] = functools.partial(case_sort, 'sort_ties_b64', TIE_SIZES, 2, values=(0.5, 1.0, 1.5))
BUILDERS['ownership'] = case_ownership
for _m in (1, 100, 127, 128):
    BUILDERS['clusters_max_det_{}'.format(_m)] = functools.partial(case_clusters, _m)
for _p in range(len(PAIR_OVERLAPS)):
    for _w in THRESHOLDS:
        BUILDERS['pair_lds_{}_{}'.format(_p, _w)] = functools.partial(case_pair_lds, _p, _w)
for _g in range(len(GLOBAL_PAIRS)):
    for _w in THRESHOLDS:
        BUILDERS['pair_global_{}_{}'.format(_g, _w)] = functools.partial(case_pair_global, _g, _w)
BUILDERS['identical_thr_one'] = functools.partial(case_identical, 'one')
BUILDERS['identical_thr_below_one'] = functools.partial(case_identical, 'below_one')
BUILDERS['zero_area'] = case_zero_area
BUILDERS['inverted_corners'] = case_inverted
BUILDERS['no_nms'] = case_no_nms
PRE_NAMES = ('pre_exactly_8192', 'pre_8193', 'pre_top_bin_overflows', 'pre_small_top_fallback', 'pre_small_top_enough',
             'pre_prefix_exactly_max_det', 'pre_prefix_one_short', 'pre_bin0_clamps', 'pre_score_one')
for _n in PRE_NAMES:                                          # (built on demand: the bins' logits come from a sweep of the oracle's sigmoid)
    BUILDERS[_n] = functools.partial(lambda n: pre_cases()[n](), _n)
BUILDERS['nonfinite'] = functools.partial(case_nonfinite, False)
BUILDERS['nonfinite_osf'] = functools.partial(case_nonfinite, True)
BUILDERS['four_full_lists'] = case_four_full_lists
NAMES = list(BUILDERS)

# one case per path, for the run through the separately enqueued stages
STAGED = {'lds': 'ownership', 'prefix': 'pre_exactly_8192', 'prefix+fallback': 'pre_prefix_one_short', 'fallback': 'pre_top_bin_overflows'}


@functools.lru_cache(maxsize=None)
def get(name):
    case = BUILDERS[name]()
    assert case.name == name
    return case


@functools.lru_cache(maxsize=None)
def census_of(name):
    return census(get(name))
