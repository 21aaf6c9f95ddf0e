""" The loop-written oracle of the cuboid NMS (include/gpp.h, gpp_cuboid_nms_f64): plain Python floats, one pair
at a time and one rank at a time.  It shares no code with utils/cuboid_nms.py or utils/kitti_eval.py.  Also the scenes both test files
use (tests/test_cuboid_nms_cpu.py, tests/test_cuboid_nms_gpu.py). """
import math

import numpy as np

COLS = 36
SCORE, ORIENT, W_, L_, X_, Z_, H_, Y_, RY_ = 12, 14, 17, 18, 19, 21, 30, 31, 32


# ---------------------------------------------------------------------------------------------------- the oracle
def corners(l, w, x, z, ry):
    """ (+,+) (-,+) (-,-) (+,-) of (l/2, w/2), rotated by r_y and shifted: counter-clockwise in (X, Z) """
    c, s = math.cos(ry), math.sin(ry)
    out = []
    for sx, sz in ((1.0, 1.0), (-1.0, 1.0), (-1.0, -1.0), (1.0, -1.0)):
        px, pz = sx * (l / 2.0), sz * (w / 2.0)
        out.append((c * px + s * pz + x, -s * px + c * pz + z))
    return out


def clip(poly, a, b):
    """ the part of the polygon on the left of the line a -> b (Sutherland-Hodgman, one edge) """
    ex, ez = b[0] - a[0], b[1] - a[1]
    out = []
    for i in range(len(poly)):
        p, q = poly[i], poly[(i + 1) % len(poly)]
        dp = ex * (p[1] - a[1]) - ez * (p[0] - a[0])
        dq = ex * (q[1] - a[1]) - ez * (q[0] - a[0])
        if dp >= 0.0:
            out.append(p)
        if (dp >= 0.0) != (dq >= 0.0):
            out.append(((p[0] * dq - q[0] * dp) / (dq - dp), (p[1] * dq - q[1] * dp) / (dq - dp)))
    return out


def area(poly):
    if len(poly) < 3:
        return 0.0
    twice = 0.0
    for i in range(len(poly)):
        p, q = poly[i], poly[(i + 1) % len(poly)]
        twice = twice + (p[0] * q[1] - q[0] * p[1])
    return abs(twice) / 2.0


def overlap(ri, rj, metric):
    """ the overlap of two live rows, ri the one with the lower row index: its rectangle is clipped against rj's edges """
    a = [float(ri[k]) for k in range(COLS)]
    b = [float(rj[k]) for k in range(COLS)]
    if any(math.isnan(v[k]) for v in (a, b) for k in (W_, L_, X_, Z_, RY_)):
        return float('nan')
    poly = corners(a[L_], a[W_], a[X_], a[Z_], a[RY_])
    g = corners(b[L_], b[W_], b[X_], b[Z_], b[RY_])
    for e in range(4):
        poly = clip(poly, g[e], g[(e + 1) % 4])
    inter = area(poly)
    area_a, area_b = a[L_] * a[W_], b[L_] * b[W_]
    if metric == 'bev':
        return inter / (area_a + area_b - inter) if area_a + area_b - inter != 0.0 else float('nan')
    if any(math.isnan(v[k]) for v in (a, b) for k in (H_, Y_)):
        return float('nan')
    hh = max(0.0, min(a[Y_], b[Y_]) - max(a[Y_] - a[H_], b[Y_] - b[H_]))
    iv = inter * hh
    den = area_a * a[H_] + area_b * b[H_] - iv
    return iv / den if den != 0.0 else float('nan')


def overlap_table(rows, metric):
    """ {(i, j): overlap} for the live rows i < j """
    live = [d for d in range(len(rows)) if float(rows[d][ORIENT]) >= 0.0]
    return {(i, j): overlap(rows[i], rows[j], metric) for n, i in enumerate(live) for j in live[n + 1:]}


def suppress(rows, metric, threshold, table=None):
    """ -> (rows_out (D, 36) float32, count, suppressor [D]) """
    rows = np.asarray(rows, np.float32)
    table = overlap_table(rows, metric) if table is None else table
    live = [d for d in range(len(rows)) if float(rows[d][ORIENT]) >= 0.0]

    def score(d):
        s = float(rows[d][SCORE])
        return -math.inf if math.isnan(s) else s
    order = sorted(live, key=lambda d: (-score(d), d))
    kept, suppressor = [], [-1] * len(rows)
    out = rows.copy()
    for d in order:                                           # one rank at a time
        for k in kept:                                        # (in rank order: the first hit is the suppressor)
            if table[(min(d, k), max(d, k))] > threshold:
                suppressor[d] = k
                break
        if suppressor[d] < 0:
            kept.append(d)
        else:
            for c in range(COLS):
                out[d][c] = -1.0
    return out, len(kept), suppressor


def margin(table, threshold):
    """ the smallest distance of an overlap of the table from the threshold (NaN overlaps aside) """
    return min([abs(o - threshold) for o in table.values() if not math.isnan(o)] + [math.inf])


# ---------------------------------------------------------------------------------------------------- the scenes
def row(score, x, z, l=3.0, w=2.0, ry=0.0, h=1.5, y=1.65, orient=0):
    r = np.zeros(COLS, np.float32)
    r[0:4] = (100.0, 100.0, 200.0, 180.0)
    r[SCORE], r[13], r[ORIENT], r[15] = score, 0, orient, 0.01
    r[16], r[W_], r[L_], r[X_], r[20], r[Z_] = h, w, l, x, y, z
    r[25] = 0.25
    r[26:30] = (100.0, 100.0, 200.0, 180.0)
    r[H_], r[Y_], r[RY_] = h, y, ry
    return r


def padding(n=1):
    return np.full((n, COLS), -1.0, np.float32)


def nan_row(score, x, z):
    r = row(score, x, z)
    r[19:26] = np.nan
    r[30:33] = np.nan
    return r


def cluster_scene(seed, clusters=10, copies=4):
    """ `clusters` cars with random r_y, each with `copies` - 1 jittered copies, the rows in random order with random scores """
    rng = np.random.default_rng(seed)
    rows = []
    for c in range(clusters):
        x, z, ry = -30.0 + 6.5 * c + rng.uniform(-0.5, 0.5), rng.uniform(8.0, 60.0), rng.uniform(-math.pi, math.pi)
        l, w, h = rng.uniform(3.4, 4.8), rng.uniform(1.5, 1.9), rng.uniform(1.4, 1.8)
        for _ in range(copies):
            rows.append(row(rng.uniform(0.06, 1.0), x + rng.normal(0.0, 0.25), z + rng.normal(0.0, 0.25), l * rng.uniform(0.95, 1.05),
                            w * rng.uniform(0.95, 1.05), ry + rng.normal(0.0, 0.08), h * rng.uniform(0.95, 1.05), 1.65 + rng.normal(0.0, 0.05),
                            int(rng.integers(0, 4))))
    return np.stack([rows[k] for k in rng.permutation(len(rows))])


CLUSTER_SEEDS = (101, 102, 103)           # chosen on the CPU: no oracle overlap within 1e-6 of CLUSTER_THRESHOLD, either metric
CLUSTER_THRESHOLD = 0.3


def small_cases():
    """ cases (i) - (vii): [(name, rows (D, 36), metric, threshold)].  r_y = 0 with dyadic sizes makes every overlap exact; elsewhere
    the overlaps leave margins far beyond an ulp of cos / sin """
    below = float(np.nextafter(0.5, 0.0))
    two = np.stack([row(0.9, 0.0, 20.0), row(0.8, 1.0, 20.0)])                       # intersection 4, union 8: exactly 0.5
    chain = np.stack([row(0.9, 0.0, 20.0), row(0.8, 1.0, 20.0), row(0.7, 2.0, 20.0)])     # A-B, B-C 0.5; A-C 0.2
    equal = np.stack([row(0.5, 0.0, 20.0), row(0.5, 0.5, 20.0), row(0.5, 10.0, 20.0), row(0.5, 10.5, 20.0)])
    unsorted = np.stack([row(0.3, 1.0, 20.0, ry=0.3), row(0.9, 0.5, 30.0, ry=-1.2), row(0.6, 0.0, 20.0, ry=0.3), row(0.95, 1.0, 20.3, ry=0.35),
                         row(0.2, 0.6, 30.1, ry=-1.1), row(0.5, 12.0, 12.0, ry=2.0)])
    bridge = np.stack([row(0.9, 0.0, 20.0), row(0.8, 0.25, 20.0, y=-6.0)])
    with_nan = np.stack([row(0.9, 0.0, 20.0), nan_row(0.85, 0.1, 20.0), row(0.8, 0.25, 20.0)])
    mixed = np.concatenate([padding(1), chain[:1], padding(2), chain[1:2], padding(1), chain[2:], padding(3)])
    rng = np.random.default_rng(7)
    full = np.stack([row(rng.uniform(0.1, 1.0), 8.0 * (k // 4) + rng.uniform(-0.4, 0.4), 20.0 + rng.uniform(-0.4, 0.4),
                         ry=rng.uniform(-0.1, 0.1) + 0.5 * (k // 4)) for k in range(128)])
    cases = []
    for metric in ('bev', '3d'):
        cases += [('exact_at_the_threshold', two, metric, 0.5), ('exact_just_below', two, metric, below),
                  ('chain', chain, metric, 0.4), ('equal_scores', equal, metric, 0.4), ('unsorted', unsorted, metric, 0.3),
                  ('bridge', bridge, metric, 0.5), ('nan_row_between', with_nan, metric, 0.5), ('padding_interleaved', mixed, metric, 0.4),
                  ('all_padding', padding(5), metric, 0.4), ('one_row', two[:1], metric, 0.4), ('d128', full, metric, 0.35)]
    return cases


def cluster_cases():
    """ case (viii): three seeded images of D = 40, both metrics """
    return [('clusters_s{}'.format(seed), cluster_scene(seed), metric, CLUSTER_THRESHOLD) for seed in CLUSTER_SEEDS for metric in ('bev', '3d')]
