"""
Constructed inputs for the plane selection of polling (csrc/poll.hip), and the census that says which branch each one reaches.

The oracles (oracle/polling_np.py, oracle/polling.c) select the naive way: R' for every plane, first argmin.  The kernel runs a
one-pass state machine per lane (level, rmin, imin, i100), merges 256 lanes over four wavefronts, resolves four ways and exists in three
forms (1, 2 or 4 planes per loop iteration, chosen by N).  Random scenes end in `rmin < 100 -> imin` with the answer anywhere; the
builders here aim at the rest.  Every builder is deterministic (the 22k database and seeded synthetic detections), returns a Case and
states, as `claims`, the property the REFERENCE must show on it; tests/test_polling_selection_cpu.py asserts the claims on
oracle/polling_np.py (so a builder that stops producing its branch fails there, not silently on the GPU), and
tests/test_polling_selection_gpu.py runs every case through the kernel against oracle/polling.c.

Nothing here imports the product path.
"""
import functools

import numpy as np

from oracle import polling_np
from keras_retinanet_3D.utils import synthetic

F = np.float32
LANES = 256                   # threads of a detection's workgroup (4 wavefronts of 64)
WAVE = 64
SENTINEL_RESIDUAL = F(100.0) / F(6.0)

# the N of every form of the kernel; the odd ones leave the last loop iteration of a 2- or 4-plane form with 1, 2 or 3 slots past the end
SIZES = {1: (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1023),
         2: (1024, 1025, 1279, 1281, 1535, 1537, 2047, 2049, 4095),
         4: (4096, 4097, 4351, 4353, 4863, 5119, 5121, 6143)}
FORM_N = (1000, 1500, 3000, 5000)   # cases a-d run at these: 1 plane per iteration, 2 (twice: 1500 >= 4 * 256 is a 2-plane size), 4
SIZE_WITH_ONE_ROW = 1025      # the sizes case that runs D = 1


def unroll_for(n):
    """ planes per loop iteration, as gpp_poll_f32 chooses it from N """
    return 4 if n >= 16 * LANES else (2 if n >= 4 * LANES else 1)


def position(index, n):
    """ where the kernel meets plane `index` of an N-plane database: (lane, wavefront, loop iteration, slot of the iteration) """
    u = unroll_for(n)
    lane = index % LANES
    return lane, lane // WAVE, index // (LANES * u), (index // LANES) % u


class Case(object):
    """ inputs of one call, its threshold, and the claims on single rows: dicts with `row` = (b, i) and any of
        index          the reference's plane index
        final          the class of the final resolution (see census)
        residual       the returned residual
        min_index      the index is above this
        wave / wave_not / min_iteration     where the kernel meets the answer
        min_rises / max_rises    level rises of the row along its busiest lane
        rises_on_lane  (lane, n): that lane meets a higher level at least n times after its first plane
        votes_all      every plane has this many votes
        stale_minimum_on_lane    lane: before the answer that lane meets a plane of a LOWER level (zc >= 0) with a smaller residual sum """

    def __init__(self, name, d, planes, thr=0.7, claims=()):
        self.name = name
        self.boxes = np.array(d['boxes'], F, order='C')
        self.dimensions = np.array(d['dimensions'], F, order='C')
        self.orientations = np.array(d['orientations'], np.int32, order='C')
        self.P_inv = np.array(d['P_inv'], F, order='C')
        self.planes = np.array(planes, F, order='C')                # (copies: the builders share cached arrays)
        self.thr = thr
        self.claims = list(claims)
        self._numpy = None
        for a in (self.boxes, self.dimensions, self.orientations, self.P_inv, self.planes):
            a.setflags(write=False)

    @property
    def N(self):
        return self.planes.shape[-2]

    def args(self):
        return self.boxes, self.dimensions, self.orientations, self.P_inv, self.planes

    def planes_batched(self):
        B = self.boxes.shape[0]
        return self.planes if self.planes.ndim == 3 else np.tile(self.planes[None], (B, 1, 1))

    def numpy_oracle(self):
        """ [keypoints, keyplanes, residuals, index] of oracle/polling_np.py, computed once """
        if self._numpy is None:
            with np.errstate(all='ignore'):
                self._numpy = polling_np.fit_road_planes(self.boxes, self.dimensions, self.orientations, self.P_inv, self.planes_batched(),
                                                         return_index=True, threshold=self.thr)
        return self._numpy


def census(case):
    """ What the reference shows on a case, per row (arrays (B, D)), from oracle/polling_np.py's table of votes, residual sums and zc:
        index   the literal rule: R' = 100 where votes < max or zc < 0, first argmin, NaN / inf never win, 0 if nothing finite
        rmin, imin    the lexicographic minimum over the planes that keep their residual;  i100 the first plane that carries the sentinel
        final   lt100 | eq100_sentinel_first | eq100_imin_first | eq100_no_sentinel | gt100_sentinel | nonfinite_sentinel |
                gt100_no_sentinel | nothing
        model_index   the answer the one-pass resolution derives from (rmin, imin, i100): equals index if the derivation is right
        rises   (B, D, 256): how often each lane meets a higher level after its first plane
        votes   (B, D, N) """
    with np.errstate(all='ignore'):                           # NaN planes and rows are among the cases
        _, _, zc, votes, res = polling_np.poll_table(case.boxes, case.dimensions, case.orientations, case.P_inv, case.planes_batched(), case.thr)
    B, D, N = votes.shape
    vmax = votes.max(axis=2, keepdims=True)
    sentinel = (votes < vmax) | (zc < 0)
    masked = np.where(sentinel, F(100.0), res).astype(F)
    key = np.where(masked < np.finfo(F).max, masked, np.inf)
    index = key.argmin(axis=2)
    index = np.where(np.isinf(key.min(axis=2)), 0, index)

    own = np.where(~sentinel & (res < np.finfo(F).max), res, np.inf)
    rmin = own.min(axis=2)
    imin = np.where(np.isinf(rmin), -1, own.argmin(axis=2))
    has100 = sentinel.any(axis=2)
    i100 = np.where(has100, sentinel.argmax(axis=2), -1)
    final = np.empty((B, D), dtype=object)
    model = np.zeros((B, D), dtype=np.int64)
    for b in range(B):
        for i in range(D):
            r, s = rmin[b, i], has100[b, i]
            if r < 100.0:
                final[b, i], model[b, i] = 'lt100', imin[b, i]
            elif r == 100.0:
                if not s:
                    final[b, i], model[b, i] = 'eq100_no_sentinel', imin[b, i]
                elif i100[b, i] < imin[b, i]:
                    final[b, i], model[b, i] = 'eq100_sentinel_first', i100[b, i]
                else:
                    final[b, i], model[b, i] = 'eq100_imin_first', imin[b, i]
            elif s:
                final[b, i], model[b, i] = ('gt100_sentinel' if np.isfinite(r) else 'nonfinite_sentinel'), i100[b, i]
            elif np.isfinite(r):
                final[b, i], model[b, i] = 'gt100_no_sentinel', imin[b, i]
            else:
                final[b, i], model[b, i] = 'nothing', 0

    rounds = -(-N // LANES)
    padded = np.full((B, D, rounds * LANES), -1.0, F)
    padded[:, :, :N] = votes
    seq = padded.reshape(B, D, rounds, LANES)
    before = np.maximum.accumulate(seq, axis=2)
    rises = (seq[:, :, 1:] > before[:, :, :-1]).sum(axis=2)
    return {'index': index, 'final': final, 'model_index': model, 'rmin': rmin, 'imin': imin, 'i100': i100, 'rises': rises, 'votes': votes,
            'res': res, 'zc': zc}


def failed_claims(case, cen):
    """ the claims of a case that the census does not bear out, as readable strings (empty = all hold) """
    bad = []
    for c in case.claims:
        b, i = c['row']
        idx = int(cen['index'][b, i])
        lane, wave, iteration, _ = position(idx, case.N)
        checks = {
            'index': lambda v: idx == v,
            'final': lambda v: cen['final'][b, i] == v,
            'residual': lambda v: case.numpy_oracle()[2][b, i] == v,
            'min_index': lambda v: idx > v,
            'wave': lambda v: wave == v,
            'wave_not': lambda v: wave != v,
            'min_iteration': lambda v: iteration >= v,
            'min_rises': lambda v: int(cen['rises'][b, i].max()) >= v,
            'max_rises': lambda v: int(cen['rises'][b, i].max()) <= v,
            'rises_on_lane': lambda v: int(cen['rises'][b, i, v[0]]) >= v[1],
            'votes_all': lambda v: bool(np.all(cen['votes'][b, i] == v)),
            'stale_minimum_on_lane': lambda v: any(cen['votes'][b, i, j] < cen['votes'][b, i, idx] and cen['zc'][b, i, j] >= 0 and
                                                   cen['res'][b, i, j] < cen['res'][b, i, idx] for j in range(v, idx, LANES)),
        }
        for k, v in c.items():
            if k != 'row' and not checks[k](v):
                bad.append('{} row {}: {} = {!r} does not hold (index {}, final {}, lane {}, wave {}, iteration {}, rises {})'.format(
                    case.name, (b, i), k, v, idx, cen['final'][b, i], lane, wave, iteration, int(cen['rises'][b, i].max())))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------- inputs

@functools.lru_cache(maxsize=None)
def base22():
    planes = synthetic.load_plane_database('22k').astype(F)
    planes.setflags(write=False)
    return planes


def batch(images, dets, seed, num_valid=None):
    d = synthetic.synthetic_polling_batch(base22(), batch=images, num_dets=dets, num_valid=num_valid, seed=seed)
    return {k: d[k] for k in ('boxes', 'dimensions', 'orientations', 'P_inv', 'true_plane')}


def tile_images(d, images):
    """ the first image of a batch, `images` times """
    return {k: np.repeat(v[:1], images, axis=0) for k, v in d.items()}


def row_table(d, b, i, planes, thr=0.7):
    """ votes, residual sums and zc (N,) of row (b, i) of a batch over planes (N, 4) """
    _, _, zc, votes, res = polling_np.poll_table(d['boxes'][b:b + 1, i:i + 1], d['dimensions'][b:b + 1, i:i + 1], d['orientations'][b:b + 1, i:i + 1],
                                                 d['P_inv'][b:b + 1], np.asarray(planes, F)[None], thr)
    return votes[0, 0], res[0, 0], zc[0, 0]


def literal_index(votes, res, zc):
    masked = np.where((votes < votes.max()) | (zc < 0), F(100.0), res)
    key = np.where(masked < np.finfo(F).max, masked, np.inf)
    return int(key.argmin()) if np.isfinite(key.min()) else 0


@functools.lru_cache(maxsize=None)
def gold_of(seed, dets, b, i):
    """ (batch, the reference's best plane of the 22k database for row (b, i) = 'gold', the planes of the database that poll below
    gold's level for that row, in database order) """
    d = batch(b + 1, dets, seed)
    votes, res, zc = row_table(d, b, i, base22())
    gold = literal_index(votes, res, zc)
    assert votes[gold] == votes.max() and zc[gold] >= 0 and res[gold] < 100.0
    return d, base22()[gold], base22()[votes < votes.max()]


def planted(filler, gold, positions, n):
    """ (n, 4): gold at every one of `positions`, the first planes of `filler` elsewhere, in order """
    positions = sorted(set(int(p) for p in positions))
    assert 0 <= positions[0] and positions[-1] < n and filler.shape[0] >= n - len(positions)
    out = np.empty((n, 4), F)
    at = np.zeros(n, bool)
    at[positions] = True
    out[at] = gold
    out[~at] = filler[:n - len(positions)]
    return out


KEY_SEED = 31


def case_planted(n):
    """ a. one plane at the maximum level, at position p: the answer is p.  The positions are the images of one batched database """
    d, gold, filler = gold_of(KEY_SEED, 2, 0, 0)
    pos = sorted({p for p in (0, 1, 63, 64, 255, 256, 257, 511, 512, 1023, 1024, n - 257, n - 2, n - 1) if p < n})
    planes = np.stack([planted(filler, gold, [p], n) for p in pos])
    claims = [{'row': (k, 0), 'index': p, 'final': 'lt100'} for k, p in enumerate(pos)]
    return Case('planted_{}'.format(n), tile_images(d, len(pos)), planes, claims=claims)


def case_duplicated(n):
    """ b. gold at several positions in different lanes, wavefronts and iterations: the lowest index wins """
    d, gold, filler = gold_of(KEY_SEED, 2, 0, 0)
    stride = LANES * unroll_for(n)
    low = stride + 3 * WAVE + 5                                   # second loop iteration, wavefront 3
    sets = [([n - 1, 300, 70], {}),
            ([n - 1, low + stride - 3 * WAVE, low], {'wave': 3, 'min_iteration': 1}),      # the later copies: wavefront 0 of the next iteration, the last plane
            ([70, 70 + LANES, 70 + 2 * LANES], {}),                                       # one lane, three rounds
            ([n - 1, 900, 650], {'wave': 2}),
            ([n - 2, n - 1], {})]
    planes = np.stack([planted(filler, gold, s, n) for s, _ in sets])
    claims = [dict({'row': (k, 0), 'index': min(s), 'final': 'lt100'}, **extra) for k, (s, extra) in enumerate(sets)]
    return Case('duplicated_{}'.format(n), tile_images(d, len(sets)), planes, claims=claims)


def case_staircase(n):
    """ c. the database sorted by one row's votes (stable): ascending, a lane meets a higher level again and again and has to forget what it
    held; descending, never.  The other rows of the batch see an arbitrary order """
    d = batch(1, 6, KEY_SEED)
    planes = base22()[:n]
    votes, _, _ = row_table(d, 0, 0, planes)
    up = planes[np.argsort(votes, kind='stable')]
    down = planes[np.argsort(-votes, kind='stable')]
    claims = [{'row': (0, 0), 'final': 'lt100', 'min_rises': 3, 'min_index': n - 1 - int((votes == votes.max()).sum())},
              {'row': (1, 0), 'final': 'lt100', 'max_rises': 0}]
    return Case('staircase_{}'.format(n), tile_images(d, 2), np.stack([up, down]), claims=claims)


def case_stale_minimum(n):
    """ c'. at a threshold low enough that votes and residual sum part ways, the plane L with the smallest residual sum of the whole
    database polls BELOW the maximum level.  L at 137, the only maximum-level plane at 137 + 256, the same lane one round later: the lane
    has to forget L's residual when it rises (in the sorted staircase a stale minimum never beats the maximum level's) """
    d = batch(1, 2, KEY_SEED)
    for thr in (0.3, 0.2, 0.1, 0.05, 0.02, 0.01):
        votes, res, zc = row_table(d, 0, 0, base22(), thr)
        gold = literal_index(votes, res, zc)
        low = int(np.where((zc >= 0) & (votes < votes.max()), res, np.inf).argmin())
        if res[low] < res[gold] < 100.0 and zc[gold] >= 0:
            break
    else:
        raise AssertionError('no threshold puts the smallest residual sum below the maximum level')
    q = 2 * WAVE + 9
    planes = planted(base22()[votes < votes.max()], base22()[gold], [q + LANES], n)
    planes[q] = base22()[low]
    claims = [{'row': (0, 0), 'index': q + LANES, 'final': 'lt100', 'wave': 2, 'rises_on_lane': (q, 1), 'stale_minimum_on_lane': q}]
    return Case('stale_minimum_{}'.format(n), d, planes[None], thr=thr, claims=claims)


TALL = 300.0


def tall_batch(seed, dets):
    d = batch(1, dets, seed)
    d['dimensions'][:, :, 0] = TALL
    return d


@functools.lru_cache(maxsize=None)
def tall_rows(n):
    """ rows of a batch of 300 m tall boxes, each with the first n planes of the database on which its zc >= 0, maximum level first (stable),
    whose count K of maximum-level planes puts the first lower plane beyond index 256, outside wavefront 0 and 256 planes before the end """
    for seed in range(40, 48):
        d = tall_batch(seed, 8)
        rows = []
        for i in range(8):
            _, _, zc = row_table(d, 0, i, base22())
            planes = base22()[zc >= 0][:n]
            votes, res, _ = row_table(d, 0, i, planes)
            top = votes == votes.max()
            K = int(top.sum())
            if planes.shape[0] == n and K > LANES and position(K, n)[1] != 0 and K + LANES < n and res[top].min() > 100.0:
                rows.append((i, planes[np.argsort(~top, kind='stable')], planes[np.argsort(top, kind='stable')], K))
        if len(rows) >= 2:
            return d, rows[:2]
    raise AssertionError('no batch of tall boxes puts two answers beyond index 256 outside wavefront 0 at N = {}'.format(n))


def case_sentinel_wins(n):
    """ d. every residual at the maximum level is > 100 (a 300 m tall box), so the first plane that carries the sentinel wins.
    Images 0, 1: maximum level first -> the answer is their count K.  Image 2: maximum level last -> plane 0, which its lane saw before
    it rose.  Image 3: 200 maximum-level planes, 256 lower ones, the other maximum-level planes, the other lower ones: the answer is
    200, in wavefront 3, and its lane rises (plane 456) after it met the answer (only an answer below 256, the first plane of its lane,
    can be followed by a rise: a later plane of a lane is either behind a lower one, which wins, or behind a maximum-level one) """
    d, rows = tall_rows(n)
    images, claims = [], []
    for i, first, last, K in rows:
        claims.append({'row': (len(images), i), 'index': K, 'final': 'gt100_sentinel', 'min_index': LANES, 'wave_not': 0, 'residual': SENTINEL_RESIDUAL})
        images.append(first)
    i, first, last, K = rows[0]
    claims.append({'row': (len(images), i), 'index': 0, 'final': 'gt100_sentinel', 'rises_on_lane': (0, 1), 'residual': SENTINEL_RESIDUAL})
    images.append(last)
    t = 3 * WAVE + 8
    moved = np.concatenate([first[:t], first[K:K + LANES], first[t:K], first[K + LANES:]])
    claims.append({'row': (len(images), i), 'index': t, 'final': 'gt100_sentinel', 'rises_on_lane': (t, 1), 'wave': 3, 'residual': SENTINEL_RESIDUAL})
    images.append(moved)
    return Case('sentinel_wins_{}'.format(n), tile_images(d, len(images)), np.stack(images), claims=claims)


def case_all_over_100():
    """ e. the tall box with a threshold nothing misses: every plane has 6 votes, no plane carries the sentinel (database filtered to
    zc >= 0 for row 0), every residual is > 100: the plain first argmin """
    d = tall_batch(40, 6)
    _, _, zc = row_table(d, 0, 0, base22(), thr=1e9)
    planes = base22()[zc >= 0][:1500]
    return Case('all_over_100', d, planes, thr=1e9, claims=[{'row': (0, 0), 'final': 'gt100_no_sentinel', 'votes_all': 6.0}])


@functools.lru_cache(maxsize=None)
def exact_100_rows():
    """ rows with orientation -1 (only the targets h and wl are non-zero, and only h depends on the height) on their own plane P, with
    the float32 height at which the residual sum of P is exactly 100.0: (batch with those heights, [(row, P)]).  P keeps one vote (wl) """
    d = batch(1, 6, 52)
    d['orientations'][:] = -1
    found = []
    for i in range(6):
        P = base22()[int(d['true_plane'][0, i])]
        one = {k: v[:, i:i + 1].copy() if k != 'P_inv' else v for k, v in d.items()}
        one['dimensions'][0, 0, 0] = 90.0
        votes, res, zc = row_table(one, 0, 0, P[None])
        if not (votes[0] == 1 and zc[0] >= 0):
            continue
        h0 = F(90.0 - (float(res[0]) - 100.0))
        assert 64.0 < h0 < 128.0                             # one binade: the 8193 float32 neighbours of the estimate are h0 + k ulp, exactly
        hs = (np.float64(h0) + np.arange(-4096, 4097) * np.float64(np.spacing(h0))).astype(F)
        many = {k: (np.repeat(v, hs.size, axis=1) if k != 'P_inv' else v) for k, v in one.items()}
        many['dimensions'][0, :, 0] = hs
        _, _, _, vv, rr = polling_np.poll_table(many['boxes'], many['dimensions'], many['orientations'], many['P_inv'], P[None, None])
        hit = np.flatnonzero((rr[0, :, 0] == F(100.0)) & (vv[0, :, 0] == 1))
        if hit.size:
            d['dimensions'][0, i, 0] = many['dimensions'][0, hit[0], 0]
            found.append((i, P))
    assert len(found) >= 2, 'fewer than two rows reach a residual sum of exactly 100.0'
    return d, found[:2]


def case_exact_100():
    """ f. a plane P at the maximum level whose residual sum is exactly 100.0, so it ties with the sentinel and the lower INDEX decides.
    Q: P pushed a few per cent further away, same level, residual > 100.  S: P fifty times further away, no vote: carries the sentinel.
    Per row three 600-plane images: a sentinel before P (the sentinel's index wins), sentinels only behind P (P wins), none at all (P) """
    d, found = exact_100_rows()
    images, claims = [], []
    for i, P in found:
        k = np.arange(600, dtype=np.float64)
        Q = np.tile(P.astype(np.float64), (600, 1))
        Q[:, 3] *= 1.02 + 1e-4 * k
        S = np.tile(P.astype(np.float64), (600, 1))
        S[:, 3] *= 50.0 + k
        Q, S = Q.astype(F), S.astype(F)
        first = Q.copy(); first[200] = S[200]; first[450] = P; first[451:] = S[451:]
        claims.append({'row': (len(images), i), 'index': 200, 'final': 'eq100_sentinel_first', 'wave': 3, 'residual': SENTINEL_RESIDUAL})
        images.append(first)
        behind = Q.copy(); behind[330] = P; behind[331:] = S[331:]
        claims.append({'row': (len(images), i), 'index': 330, 'final': 'eq100_imin_first', 'wave': 1, 'min_iteration': 1, 'residual': SENTINEL_RESIDUAL})
        images.append(behind)
        none = Q.copy(); none[330] = P
        claims.append({'row': (len(images), i), 'index': 330, 'final': 'eq100_no_sentinel', 'residual': SENTINEL_RESIDUAL})
        images.append(none)
    return Case('exact_100', tile_images(d, len(images)), np.stack(images), claims=claims)


def case_nan_planes():
    """ g. a plane with b == 0 canonicalises to NaN, and a NaN plane has 6 votes (`r > thr` is false): for a row whose real maximum is
    below 6 (orientation -1) every real plane drops to the sentinel and the first real plane wins.  Plane 259 is the second plane of
    the lane that holds the answer, 3: that lane rises after it met the answer """
    d = batch(2, 6, 61)
    d['orientations'][:, :3] = -1
    planes = base22()[:1500].copy()
    planes[[0, 1, 2, 259, 700], 1] = 0.0
    claims = [{'row': (b, i), 'index': 3, 'final': 'nonfinite_sentinel', 'residual': SENTINEL_RESIDUAL, 'rises_on_lane': (3, 1)}
              for b in range(2) for i in range(3)]
    return Case('nan_planes', d, planes, claims=claims)


def case_all_nan_planes():
    d = batch(2, 6, 61)
    planes = base22()[:300].copy()
    planes[:, 1] = 0.0
    return Case('all_nan_planes', d, planes, claims=[{'row': (b, i), 'index': 0, 'final': 'nothing'} for b in range(2) for i in range(6)])


def case_nan_rows():
    """ g. a NaN and an inf keypoint coordinate (rows (0, 2) and (0, 3)): every residual sum is NaN, but the segments without that keypoint
    still vote, so lower planes exist and the first of them, plane 0, wins with the sentinel.  A NaN P_inv (image 2): nothing finite and
    nothing masked, index 0 by the fallback.  Every other row answers as it does without them """
    d = batch(3, 6, 62)
    planes = base22()[:1500]
    clean = Case('clean', d, planes).numpy_oracle()[3]
    d['boxes'][0, 2, 4] = np.nan
    d['boxes'][0, 3, 6] = np.inf
    d['P_inv'][2, 1, 1] = np.nan
    dead = [(0, 2), (0, 3)] + [(2, i) for i in range(6)]
    claims = [{'row': r, 'index': 0, 'final': 'nonfinite_sentinel', 'residual': SENTINEL_RESIDUAL} for r in dead[:2]]
    claims += [{'row': r, 'index': 0, 'final': 'nothing'} for r in dead[2:]]
    claims += [{'row': (b, i), 'index': int(clean[b, i]), 'final': 'lt100'} for b in range(2) for i in range(6) if (b, i) not in dead]
    return Case('nan_rows', d, planes, claims=claims)


def case_threshold(name, thr, votes_all):
    """ h. thresholds other than 0.7 on an ordinary batch and a database shared by the images """
    d = batch(2, 6, 71)
    claims = [] if votes_all is None else [{'row': (b, i), 'votes_all': votes_all} for b in range(2) for i in range(6)]
    return Case(name, d, base22()[:3000], thr=thr, claims=claims)


def case_size(n):
    """ i. an ordinary batch with a padding run on the first n planes (image 0), and on n planes whose LAST one is the only plane at the
    maximum level of row (1, 0) (image 1): the slot of the last loop iteration that has planes behind it past the end """
    dets = 1 if n == SIZE_WITH_ONE_ROW else 6
    d, gold, filler = gold_of(81, dets, 1, 0)
    d = {k: v.copy() for k, v in d.items()}
    if dets > 1:
        d['boxes'][:, 4:] = -1.0; d['dimensions'][:, 4:] = -1.0; d['orientations'][:, 4:] = -1
    planes = np.stack([base22()[:n], planted(filler, gold, [n - 1], n)])
    return Case('size_{}'.format(n), d, planes, claims=[{'row': (1, 0), 'index': n - 1, 'final': 'lt100'}])


BUILDERS = {}
for _n in FORM_N:
    BUILDERS['planted_{}'.format(_n)] = functools.partial(case_planted, _n)
    BUILDERS['duplicated_{}'.format(_n)] = functools.partial(case_duplicated, _n)
    BUILDERS['staircase_{}'.format(_n)] = functools.partial(case_staircase, _n)
    BUILDERS['stale_minimum_{}'.format(_n)] = functools.partial(case_stale_minimum, _n)
    BUILDERS['sentinel_wins_{}'.format(_n)] = functools.partial(case_sentinel_wins, _n)
BUILDERS['all_over_100'] = case_all_over_100
BUILDERS['exact_100'] = case_exact_100
BUILDERS['nan_planes'] = case_nan_planes
BUILDERS['all_nan_planes'] = case_all_nan_planes
BUILDERS['nan_rows'] = case_nan_rows
BUILDERS['thr_zero'] = functools.partial(case_threshold, 'thr_zero', 0.0, 0.0)
BUILDERS['thr_huge'] = functools.partial(case_threshold, 'thr_huge', 1e9, 6.0)
BUILDERS['thr_negative'] = functools.partial(case_threshold, 'thr_negative', -1.0, 0.0)
for _form in sorted(SIZES):
    for _n in SIZES[_form]:
        BUILDERS['size_{}'.format(_n)] = functools.partial(case_size, _n)
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name):
    case = BUILDERS[name]()
    assert case.name == name
    return case
