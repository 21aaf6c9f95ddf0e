""" The road-plane fit of DESIGN.md 4.22 as plain loops over Python integers (test infrastructure): nothing here is vectorised and nothing is
shared with utils/road_fit.py but the option resolution (the gates are specified as "computed once on the host and passed as doubles").

Exact quantities are Python ints.  The rule's rounded float64 operations are made from exact values: a product of two integers is rounded
by float(int * int) and a product of two doubles by float(Fraction * Fraction), both correctly rounded by Python -- what IEEE multiplication
of the exactly converted operands gives -- so no float multiplication of the code under test is repeated here.  Sums of doubles are
Python float additions (one IEEE operation each).

Also the seeded cases both test modules run (cases()), and their oracle results, computed once per process (expected()). """
import functools
import math
from fractions import Fraction

import numpy as np

from keras_retinanet_3D.utils import road_fit

M32 = 0xffffffff


# ---------------------------------------------------------------------------------------------------- the rule
def mix(u):
    u &= M32
    u ^= u >> 16
    u = (u * 0x7feb352d) & M32
    u ^= u >> 15
    u = (u * 0x846ca68b) & M32
    u ^= u >> 16
    return u


def draw(seed, frame_id, h, k, m):
    r = mix(mix(mix((seed + frame_id) & M32) + h) + k)
    return (r * m) >> 32


def rmul(a, b):
    """ the float64 product of two doubles, rounded once """
    return float(Fraction(a) * Fraction(b))


def quantise(points, T, region_q):
    """ step 1: the kept points of one scan as a list of (x, y, z) ints, in the scan's order """
    xq, yq, zq = region_q
    out = []
    for i in range(len(points)):
        x, y, z = float(points[i][0]), float(points[i][1]), float(points[i][2])
        q = []
        for r in range(3):
            t0, t1, t2, t3 = [float(T[r][k]) for k in range(4)]
            v = ((t0 * x + t1 * y) + t2 * z) + t3              # Python floats: one rounded operation each, in this order
            w = v * 256.0 + 0.5
            if not math.isfinite(w):
                q = None
                break
            q.append(math.floor(w))                            # exact: the integer below a double
        if q is None:
            continue
        if abs(q[0]) <= xq and abs(q[1]) <= yq and 1 <= q[2] <= zq:
            out.append((q[0], q[1], q[2]))
    return out


def hypothesis(q, seed, frame_id, h, o):
    """ step 2: (n, d0, nn, valid) of hypothesis h over the kept points q """
    m = len(q)
    if m < 3:
        return (0, 0, 0), 0, 0.0, False
    p0, p1, p2 = [q[draw(seed, frame_id, h, k, m)] for k in range(3)]
    a = [p1[i] - p0[i] for i in range(3)]
    b = [p2[i] - p0[i] for i in range(3)]
    n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    d0 = n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2]
    assert all(abs(v) < 2 ** 33 for v in n) and abs(d0) < 2 ** 51
    nn = (float(n[0] * n[0]) + float(n[1] * n[1])) + float(n[2] * n[2])
    dd = float(d0 * d0)
    valid = nn > 0.0 and float(n[1] * n[1]) >= rmul(o['c2'], nn) and rmul(o['hlo2'], nn) <= dd <= rmul(o['hhi2'], nn)
    return n, d0, nn, valid


def inlier(p, n, d0, t2):
    dot = n[0] * p[0] + n[1] * p[1] + n[2] * p[2] - d0
    assert abs(dot) < 2 ** 51
    return float(dot * dot) <= t2


def score(q, frame_id, o):
    """ step 3: the counts of one frame, -1 for an invalid hypothesis """
    counts = []
    for h in range(o['H']):
        n, d0, nn, valid = hypothesis(q, o['seed'], frame_id, h, o)
        if not valid:
            counts.append(-1)
            continue
        t2 = rmul(o['tq2'], nn)
        nx, ny, nz = n
        c = 0
        for x, y, z in q:
            dot = nx * x + ny * y + nz * z - d0
            if float(dot * dot) <= t2:
                c += 1
        counts.append(c)
    return counts


def winner(counts, min_inliers):
    """ step 4: (winner, inliers): the first hypothesis of the largest count """
    best, at = -1, -1
    for h, c in enumerate(counts):
        if c > best:
            best, at = c, h
    if best < 0:
        return -1, 0
    return (at if best >= min_inliers else -1), best


def moments(q, frame_id, w, o):
    """ step 5: the ten sums as Python ints """
    s = [0] * 10
    if w < 0:
        return s
    n, d0, nn, _ = hypothesis(q, o['seed'], frame_id, w, o)
    t2 = rmul(o['tq2'], nn)
    for p in q:
        if inlier(p, n, d0, t2):
            x, y, z = p
            for k, v in enumerate((1, x, y, z, x * x, x * z, z * z, x * y, z * y, y * y)):
                s[k] += v
    assert all(abs(v) < 2 ** 50 for v in s)
    return s


def fit(points_list, T_list, frame_ids, **options):
    """ every stage of every frame: dict of lists q, kept, count, winner, inliers, sums """
    o = road_fit.resolve_options(**options)
    out = {k: [] for k in ('q', 'kept', 'count', 'winner', 'inliers', 'sums')}
    for points, T, fid in zip(points_list, T_list, frame_ids):
        q = quantise(np.asarray(points, np.float32).reshape(-1, 4), np.asarray(T, np.float64).reshape(3, 4), o['region_q'])
        counts = score(q, int(fid), o)
        w, c = winner(counts, o['min_inliers'])
        for k, v in zip(('q', 'kept', 'count', 'winner', 'inliers', 'sums'), (q, len(q), counts, w, c, moments(q, int(fid), w, o))):
            out[k].append(v)
    return out


# ---------------------------------------------------------------------------------------------------- seeded clouds
PERMUTE = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])       # velodyne (x fwd, y left, z up) -> camera
# a velodyne -> camera matrix with the digits of a KITTI Tr_velo_to_cam line (R0_rect = identity): every product and sum of step 1 rounds
KITTI_T = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                    [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]])
SLAB = 512                                                     # GPP_ROAD_SLAB (include/gpp.h); the score launch has at most 64 workgroups along a frame


def to_velodyne(cam, T=PERMUTE, reflectance=0.25):
    """ camera-frame points (n, 3) float64 -> the (n, 4) float32 scan that T maps (up to float32 rounding) back onto them """
    cam = np.asarray(cam, np.float64).reshape(-1, 3)
    velo = (cam - T[:, 3]) @ np.linalg.inv(T[:, :3]).T
    return np.concatenate([velo, np.full((cam.shape[0], 1), reflectance)], axis=1).astype(np.float32)


def road_cloud(rng, n, height=1.65, slope=(0.01, -0.02), noise=0.02, clutter=0.3, x_max=25.0, z_max=60.0):
    """ n camera-frame points: a road y = height + slope . (x, z) with Gaussian noise, `clutter` of them lifted by up to 2 m, and some
    outside the default region """
    x, z = rng.uniform(-x_max, x_max, n), rng.uniform(-5.0, z_max, n)
    y = height + slope[0] * x + slope[1] * z + rng.normal(0.0, noise, n)
    lifted = rng.random(n) < clutter
    y[lifted] -= rng.uniform(0.1, 2.0, int(lifted.sum()))
    return np.stack([x, y, z], axis=1)


def dyadic_plane_cloud(rng, n, height, ax=0.0, az=0.0, x_max=15, z_max=40):
    """ n points exactly on y = height + ax x + az z (dyadic coefficients), x in halves of a metre, z in whole metres: they quantise
    without error """
    x = rng.integers(-2 * x_max, 2 * x_max + 1, n) / 2.0
    z = rng.integers(1, z_max + 1, n).astype(np.float64)
    return np.stack([x, height + ax * x + az * z, z], axis=1)


def exact_case(n=5000, seed=99):
    """ the exact-recovery cloud: y = 1.625 + x / 64 + z / 128, x in halves within +-30 m, z whole metres 1 .. 69, 30 % lifted by
    0.5 .. 2.7 m; region at the caps so that every point is kept.  Returns (case, truth plane (4,), number of plane points) """
    rng = np.random.default_rng(seed)
    cam = dyadic_plane_cloud(rng, n, 1.625, 1.0 / 64, 1.0 / 128, x_max=30, z_max=69)
    lifted = rng.random(n) < 0.3
    cam[lifted, 1] -= rng.uniform(0.5, 2.7, int(lifted.sum()))
    truth = np.array([1.0 / 64, -1.0, 1.0 / 128, 1.625]) / math.sqrt(1.0 / 64 ** 2 + 1.0 + 1.0 / 128 ** 2)
    case = ([to_velodyne(cam)], [PERMUTE], [0], dict(hypotheses=300, seed=seed, region=(40.0, 8.0, 80.0)))
    return case, truth, int((~lifted).sum())


def _ragged():
    """ scans of 0, 1, 255, 256, 257 and 5000 points in one batch: an empty scan, a scan gated out entirely, the bounds, NaN and infinity """
    rng = np.random.default_rng(5)
    q = 1.0 / 256
    bounds = np.array([[20.0, 1.0, 10.0], [20.0 + q, 1.0, 10.0], [-20.0, 1.0, 10.0], [-20.0 - q, 1.0, 10.0],
                       [3.0, 8.0, 10.0], [3.0, 8.0 + q, 10.0], [3.0, -8.0, 10.0], [3.0, -8.0 - q, 10.0],
                       [3.0, 1.0, 50.0], [3.0, 1.0, 50.0 + q], [3.0, 1.0, q], [3.0, 1.0, 0.0], [3.0, 1.0, q / 2], [3.0, 1.0, q / 2 - q / 64]])
    f4 = np.concatenate([bounds, road_cloud(rng, 257 - len(bounds))])
    f4 = to_velodyne(f4[rng.permutation(257)])
    for row, col, v in ((20, 0, np.nan), (21, 1, np.inf), (22, 2, -np.inf), (23, 0, np.inf), (24, 2, np.nan), (25, 0, 3.0e38)):
        f4[row, col] = v
    behind = road_cloud(rng, 255)
    behind[:, 2] = -np.abs(behind[:, 2]) - 1.0
    scans = [np.zeros((0, 4), np.float32), to_velodyne([[1.0, 1.5, 7.0]]), to_velodyne(behind), to_velodyne(road_cloud(rng, 256), KITTI_T),
             f4, to_velodyne(road_cloud(rng, 5000), KITTI_T)]
    Ts = [PERMUTE, PERMUTE, PERMUTE, KITTI_T, PERMUTE, KITTI_T]
    return scans, Ts, [7, 0, 4000000000, 3, 12, 5], dict(hypotheses=300, seed=3)


def _slab(H):
    """ kept one below, at and one above the score launch's slab, and frames of 0, 2 and 3 kept points (three points: most draws repeat one,
    n = 0) """
    rng = np.random.default_rng(6)
    scans = []
    for m in (SLAB - 1, SLAB, SLAB + 1, 0, 2, 3):
        cam = dyadic_plane_cloud(rng, m, 1.5, 1.0 / 128, -1.0 / 256)
        if m > 3:
            cam[::5, 1] -= rng.uniform(0.05, 1.0, cam[::5].shape[0])
        else:
            cam[:, 0], cam[:, 2] = [-4.0, 6.0, 1.5][:m], [5.0, 9.0, 30.0][:m]
            cam[:, 1] = 1.5 + cam[:, 0] / 128 - cam[:, 2] / 256
        outside = road_cloud(rng, 40)
        outside[:, 0] += 60.0                                # gated out: they move the kept points' positions in the scan, not their number
        both = np.concatenate([cam, outside])
        order = np.argsort(np.concatenate([np.arange(m) * 2.0, rng.uniform(0, max(1, 2 * m), 40)]), kind='stable')
        scans.append(to_velodyne(both[order]))
    return scans, [PERMUTE] * 6, [0, 1, 2, 3, 4, 5], dict(hypotheses=H, seed=1, min_inliers=100)


def _gates():
    """ a vertical wall (tilt gate), planes at 0.5 m and 3 m (height gate), an all-coplanar cloud (every valid hypothesis ties), and the same
    plane with fewer points than min_inliers """
    rng = np.random.default_rng(8)
    wall = np.stack([np.full(300, 3.0), rng.integers(-1024, 1025, 300) / 256.0, rng.integers(256, 8000, 300) / 256.0], axis=1)
    scans = [to_velodyne(wall), to_velodyne(dyadic_plane_cloud(rng, 300, 0.5)), to_velodyne(dyadic_plane_cloud(rng, 300, 3.0)),
             to_velodyne(dyadic_plane_cloud(rng, 600, 1.5, 1.0 / 32, 1.0 / 64)), to_velodyne(dyadic_plane_cloud(rng, 50, 1.5, 1.0 / 32, 1.0 / 64))]
    return scans, [PERMUTE] * 5, [10, 11, 12, 13, 14], dict(hypotheses=64, seed=2, min_inliers=100)


def _caps():
    """ one frame at the hard caps: coordinates at +-10 240 / +-2 048 / 20 480 quanta and between, every gate open, so that the largest cross
    products and dot products the arithmetic allows are scored """
    rng = np.random.default_rng(9)
    n = 600
    pick = lambda lo, hi: np.where(rng.random(n) < 0.6, rng.choice([lo, hi], n), rng.integers(lo, hi + 1, n))  # noqa: E731
    cam = np.stack([pick(-10240, 10240), pick(-2048, 2048), pick(1, 20480)], axis=1) / 256.0
    return [to_velodyne(cam)], [PERMUTE], [4294967295], dict(hypotheses=300, seed=4294967295, region=(40.0, 8.0, 80.0), max_tilt=90.0,
                                                             height=(0.0, 100.0), threshold=2.0, min_inliers=1)


def _long():
    """ one frame of more kept points than the score launch has workgroups along a frame (64 slabs): a workgroup walks several slabs """
    rng = np.random.default_rng(10)
    n = 64 * SLAB + 2 * SLAB + 37
    cam = dyadic_plane_cloud(rng, n, 1.75, -1.0 / 64, 1.0 / 256)
    cam[::3, 1] -= rng.uniform(0.0, 1.5, cam[::3].shape[0])
    return [to_velodyne(cam)], [PERMUTE], [77], dict(hypotheses=3, seed=6)


@functools.lru_cache(maxsize=None)
def cases():
    return {'long_h3': _long(), 'slab_h1030': _slab(1030), 'ragged': _ragged(), 'slab_h257': _slab(257), 'slab_h1': _slab(1), 'gates_h64': _gates(), 'caps': _caps(), 'exact': exact_case()[0]}


@functools.lru_cache(maxsize=None)
def expected(name):
    """ the oracle's stages of a case, once per process """
    scans, Ts, ids, options = cases()[name]
    return fit(scans, Ts, ids, **options)


def as_arrays(exp, H):
    """ the oracle's lists in the layout of road_fit.device_stages: kept, count (F, H), winner, inliers, sums (F, 10) """
    F = len(exp['kept'])
    return {'kept': np.asarray(exp['kept'], np.int32), 'count': np.asarray(exp['count'], np.int32).reshape(F, H),
            'winner': np.asarray(exp['winner'], np.int32), 'inliers': np.asarray(exp['inliers'], np.int32),
            'sums': np.asarray(exp['sums'], np.int64).reshape(F, 10)}
