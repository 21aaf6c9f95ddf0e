""" Several road planes per frame, DESIGN.md 4.24, as plain loops over Python integers (test infrastructure): the rounds, the round seed, the
peel and the validity step, on top of tests/road_fit_oracle.py (hypothesis, inlier, score, winner and moments are imported from there and
run once per round under the round's seed).  Nothing here is vectorised and nothing is shared with utils/road_fit.py but the option
resolution and solve_moments (the host's step of both forms).

Also the seeded frames both test modules run: the two-level frames, their pool, and the share-gate frame. """
import functools
import math
from fractions import Fraction

import numpy as np

import road_fit_oracle as RO
from keras_retinanet_3D.utils import road_fit

STEP = 0x9e3779b9


# ---------------------------------------------------------------------------------------------------- the rule
def round_seed(seed, r):
    return (seed + r * STEP) % (1 << 32)


def peel(q, frame_id, w, o):
    """ rule 3: the points of q (a list of int triples) that are no inliers of hypothesis w under o['seed'], in their order.  No winner: the
    frame is finished.  A plane with nn = 0 (hand-set winners only) has no inliers: gpp_road_moments adds nothing for it """
    if w < 0 or w >= o['H']:
        return []
    n, d0, nn, _ = RO.hypothesis(q, o['seed'], frame_id, w, o)
    if not nn > 0.0:
        return list(q)
    t2 = RO.rmul(o['tq2'], nn)
    out = []
    for p in q:
        if not RO.inlier(p, n, d0, t2):
            out.append(p)
    return out


def inlier_count(q, frame_id, w, o):
    """ N of gpp_road_moments for a hand-set winner: 0 without a winner and for a plane with nn = 0 """
    if w < 0 or w >= o['H']:
        return 0
    n, d0, nn, _ = RO.hypothesis(q, o['seed'], frame_id, w, o)
    if not nn > 0.0:
        return 0
    t2 = RO.rmul(o['tq2'], nn)
    return sum(1 for p in q if RO.inlier(p, n, d0, t2))


def rounds(points_list, T_list, frame_ids, P, **options):
    """ every stage of every round of every frame: a list of P dicts of lists q, kept, count, winner, inliers, sums (RO.fit's layout) """
    o = road_fit.resolve_options(**options)
    qs = [RO.quantise(np.asarray(p, np.float32).reshape(-1, 4), np.asarray(T, np.float64).reshape(3, 4), o['region_q'])
          for p, T in zip(points_list, T_list)]
    out = []
    for r in range(P):
        orr = dict(o, seed=round_seed(o['seed'], r))
        rec = {k: [] for k in ('q', 'kept', 'count', 'winner', 'inliers', 'sums')}
        nxt = []
        for q, fid in zip(qs, frame_ids):
            counts = RO.score(q, int(fid), orr)
            w, c = RO.winner(counts, o['min_inliers'])
            for k, v in zip(('q', 'kept', 'count', 'winner', 'inliers', 'sums'), (q, len(q), counts, w, c, RO.moments(q, int(fid), w, orr))):
                rec[k].append(v)
            nxt.append(peel(q, int(fid), w, orr))
        out.append(rec)
        qs = nxt
    return out


def validity(kept0, winners, inliers, sums, min_share):
    """ rule 4 for one frame: the list of P flags """
    need = math.ceil(Fraction(min_share) * kept0)
    flags, ok = [], True
    for r, (w, c, s) in enumerate(zip(winners, inliers, sums)):
        ok = ok and w >= 0 and road_fit.solve_moments(s)[0] is not None and (r == 0 or c >= need)
        flags.append(ok)
    return flags


def as_arrays(rec, H):
    return RO.as_arrays(rec, H)


# ---------------------------------------------------------------------------------------------------- seeded frames
LEVELS = 20
TWO_LEVEL_OPTIONS = dict(hypotheses=64)


def two_level_truth():
    """ the 40 planes in (frame, round) order: frame i has y = 1.25 + i / 64 and that + 0.75 """
    return np.array([[0.0, -1.0, 0.0, 1.25 + i / 64.0 + dy] for i in range(LEVELS) for dy in (0.0, 0.75)], np.float64)


@functools.lru_cache(maxsize=None)
def two_level_frames():
    """ 20 frames, frame_id = i: 400 points on y = 1.25 + i / 64 with z in 1 .. 20 and 250 points 0.75 m below them (y larger) with z in
    21 .. 40, shuffled; all from one default_rng(3).  (scans, Ts, ids, options) """
    rng = np.random.default_rng(3)
    scans = []
    for i in range(LEVELS):
        near = RO.dyadic_plane_cloud(rng, 400, 1.25 + i / 64.0, z_max=20)
        far = RO.dyadic_plane_cloud(rng, 250, 1.25 + i / 64.0 + 0.75, z_max=20)
        far[:, 2] += 20.0
        both = np.concatenate([near, far])
        scans.append(RO.to_velodyne(both[rng.permutation(650)]))
    return scans, [RO.PERMUTE] * LEVELS, list(range(LEVELS)), dict(TWO_LEVEL_OPTIONS)


@functools.lru_cache(maxsize=None)
def share_gate_frame():
    """ frame 0 of the two-level frames with 40 more coplanar points on a third level (y = 1.625, between the two and inside the height
    band; z in 1 .. 40), min_inliers 30: 690 kept points, so min_share 0.10 asks a later round for 69 inliers """
    scans, Ts, ids, options = two_level_frames()
    rng = np.random.default_rng(4)
    third = RO.to_velodyne(RO.dyadic_plane_cloud(rng, 40, 1.625))
    both = np.concatenate([scans[0], third])
    return [both[rng.permutation(690)]], [RO.PERMUTE], [0], dict(options, min_inliers=30)


@functools.lru_cache(maxsize=None)
def expected_rounds(name, P=3):
    """ the oracle's rounds of a case, once per process: 'two_level', 'share_gate' or a case of road_fit_oracle.cases() """
    if name == 'two_level':
        scans, Ts, ids, options = two_level_frames()
    elif name == 'share_gate':
        scans, Ts, ids, options = share_gate_frame()
    else:
        scans, Ts, ids, options = RO.cases()[name]
    return rounds(scans, Ts, ids, P, **options)
