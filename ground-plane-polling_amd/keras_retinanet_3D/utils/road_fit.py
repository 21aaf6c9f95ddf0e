"""
Fit a pool of road planes from LiDAR scans: per frame a consensus fit of one plane to the road region of the scan, in rectified camera
coordinates -- DESIGN.md section 4.22 is the specification.  The pool is what utils/plane_db.py distils; the reference tells users of
another dataset to "replace road_planes_database.mat with relevant files of your own" and has nothing that makes one.

    read_velodyne, read_velo_calibration   a KITTI scan and R0_rect . Tr_velo_to_cam
    fit_device     gate / quantise, score, winner and moments on the device (csrc/road_fit.hip), then solve_moments
    fit_np         the same in NumPy: equal to fit_device entry for entry, planes bit for bit
    solve_moments  ten integer sums -> the plane (host only; both forms use it)
    fit_pool       velodyne + calib directories -> the valid planes in file order, with the per-frame record
    fit_rounds_np, fit_rounds_device   several planes per frame: after a round's winner its inliers are taken out
                   of the frame's point list (peel_np / gpp_road_peel_i32) and the frame is scored again under the round's seed
    read_plane_files   the planes/NNNNNN.txt files that KITTI-derived sets distribute, as a pool

The fit is done in exact integers: a point is quantised once, at Q = 256 quanta per metre, and every later quantity is an integer below
2^53 or one rounded float64 operation on such integers, so the device result does not depend on the order of lanes or atomics.

The device entry points raise GppError without a GPU, like polling_ceiling; fit_np needs nothing but NumPy.
"""
import math
import os
from fractions import Fraction

import numpy as np

Q = 256                                                     # GPP_ROAD_Q (include/gpp.h): quanta per metre
REGION_CAPS_M = (40.0, 8.0, 80.0)                           # GPP_ROAD_MAX_XQ / YQ / ZQ in metres
MAX_POINTS = 1 << 20                                        # GPP_ROAD_MAX_POINTS: points of one scan
MAX_FRAMES = 65535                                          # frames of one device chunk
SUM_NAMES = ('N', 'Sx', 'Sy', 'Sz', 'Sxx', 'Sxz', 'Szz', 'Sxy', 'Szy', 'Syy')
DEFAULTS = dict(hypotheses=1024, threshold=0.10, region=(20.0, 8.0, 50.0), height=(1.0, 2.5), max_tilt=15.0, min_inliers=100, seed=0)
CHUNK_BYTES = 1 << 30                                       # fit_pool: device bytes of one chunk (points, q, counts)
ROUND_SEED_STEP = 0x9e3779b9                                # section 4.24: round r draws with seed + r * ROUND_SEED_STEP (mod 2^32)
MIN_SHARE = 0.10                                            # section 4.24: a later round's plane needs this share of the frame's kept points


# ---------------------------------------------------------------------------------------------------- options
def resolve_options(**options):
    """ the caller's options (DEFAULTS) -> what both forms compute with: H, seed, min_inliers, the region in quanta (xq, yq, zq) and the
    float64 gates c2 = cos^2(max tilt), hlo2 = (h_lo Q)^2, hhi2 = (h_hi Q)^2, tq2 = (threshold Q)^2, made here once so that both forms see
    the same bits """
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise ValueError('unknown option(s) {}: the fit takes {}'.format(sorted(unknown), sorted(DEFAULTS)))
    o = dict(DEFAULTS, **options)
    H, seed, min_inliers = int(o['hypotheses']), int(o['seed']), int(o['min_inliers'])
    region = [float(v) for v in o['region']]
    if len(region) != 3:
        raise ValueError('region takes three numbers (x, y, z in metres), got {}'.format(o['region']))
    rq = [int(math.floor(v * Q + 0.5)) if math.isfinite(v) else -1 for v in region]
    if rq[0] < 0 or rq[1] < 0 or rq[2] < 1 or any(v > cap * Q for v, cap in zip(rq, REGION_CAPS_M)):
        raise ValueError('region {} m: |x| <= {:g}, |y| <= {:g} and z <= {:g} m are the most the exact arithmetic takes'.format(
            tuple(region), *REGION_CAPS_M))
    lo, hi = [float(v) for v in o['height']]
    tilt, tau = float(o['max_tilt']), float(o['threshold'])
    if not (0.0 <= lo <= hi and math.isfinite(hi)):
        raise ValueError('height {} m: needs 0 <= lo <= hi'.format((lo, hi)))
    if not 0.0 <= tilt <= 90.0:
        raise ValueError('max_tilt {} degrees: needs 0 .. 90'.format(tilt))
    if not (tau >= 0.0 and math.isfinite(tau)):
        raise ValueError('threshold {} m: needs a finite value >= 0'.format(tau))
    if H < 1 or H > (1 << 20):
        raise ValueError('hypotheses {}: needs 1 .. 2^20'.format(H))
    if min_inliers < 1:
        raise ValueError('min_inliers {}: needs >= 1'.format(min_inliers))
    if not 0 <= seed < (1 << 32):
        raise ValueError('seed {}: needs 0 .. 2^32 - 1'.format(seed))
    c = math.cos(math.radians(tilt))
    return dict(H=H, seed=seed, min_inliers=min_inliers, region_q=tuple(rq), c2=min(1.0, c * c), hlo2=(lo * Q) ** 2, hhi2=(hi * Q) ** 2,
                tq2=(tau * Q) ** 2)


# ---------------------------------------------------------------------------------------------------- the rule's pieces, in NumPy
def mix(u):
    """ the 32-bit mixer on uint32 arrays (wrap-around arithmetic) """
    u = np.asarray(u, np.uint32).copy()
    u ^= u >> np.uint32(16)
    u *= np.uint32(0x7feb352d)
    u ^= u >> np.uint32(15)
    u *= np.uint32(0x846ca68b)
    u ^= u >> np.uint32(16)
    return u


def draw_indices(seed, frame_id, H, m):
    """ (H, 3) int64: the three point indices of every hypothesis of a frame with m kept points """
    with np.errstate(over='ignore'):
        key = mix(np.uint32(seed) + np.asarray([frame_id], np.uint32))
        kh = mix(key + np.arange(H, dtype=np.uint32))
        r = mix(kh[:, None] + np.arange(3, dtype=np.uint32)[None, :])
    return ((r.astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def quantise_np(points, T, region_q):
    """ step 1 on one scan: points (n, 4) float32, T (3, 4) float64 -> the kept points (m, 3) int32 in the scan's order """
    p = np.asarray(points, np.float32).reshape(-1, 4).astype(np.float64)
    T = np.asarray(T, np.float64).reshape(3, 4)
    xq, yq, zq = [float(v) for v in region_q]
    with np.errstate(invalid='ignore', over='ignore'):
        v = [np.floor((((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]) * 256.0 + 0.5) for r in range(3)]
        keep = (np.abs(v[0]) <= xq) & (np.abs(v[1]) <= yq) & (v[2] >= 1.0) & (v[2] <= zq)
    return np.stack([c[keep] for c in v], axis=1).astype(np.int32).reshape(-1, 3)


def planes_np(q, frame_id, o):
    """ step 2 on one frame's kept points q (m, 3): (n (H, 3) int64, d0 (H,) int64, nn (H,) float64, valid (H,) bool) """
    H, m = o['H'], q.shape[0]
    if m < 3:
        return np.zeros((H, 3), np.int64), np.zeros(H, np.int64), np.zeros(H), np.zeros(H, bool)
    p = q.astype(np.int64)[draw_indices(o['seed'], frame_id, H, m)]                       # (H, 3 draws, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    d0 = (n * p[:, 0]).sum(axis=1)
    nf = n.astype(np.float64)
    nn = (nf[:, 0] * nf[:, 0] + nf[:, 1] * nf[:, 1]) + nf[:, 2] * nf[:, 2]
    dd = d0.astype(np.float64) * d0.astype(np.float64)
    valid = (nn > 0.0) & (nf[:, 1] * nf[:, 1] >= o['c2'] * nn) & (o['hlo2'] * nn <= dd) & (dd <= o['hhi2'] * nn)
    return n, d0, nn, valid


def _inlier_mask(q64, n, d0, t2):
    """ points (m, 3) int64 against planes n (K, 3), d0 (K,), t2 (K,) -> (m, K) bool """
    dot = (q64 @ n.T - d0[None, :]).astype(np.float64)
    return dot * dot <= t2[None, :]


def score_np(q, frame_id, o, block=4096):
    """ steps 2-3 on one frame: count (H,) int32, -1 where the hypothesis is invalid """
    n, d0, nn, valid = planes_np(q, frame_id, o)
    count = np.full(o['H'], -1, np.int32)
    if valid.any():
        q64, t2 = q.astype(np.int64), o['tq2'] * nn[valid]
        c = np.zeros(int(valid.sum()), np.int64)
        for at in range(0, q.shape[0], block):
            c += _inlier_mask(q64[at:at + block], n[valid], d0[valid], t2).sum(axis=0)
        count[valid] = c
    return count


def winner_np(count, min_inliers):
    """ step 4: (winner, inliers) of one frame's counts: the first hypothesis of the largest count, -1 below min_inliers """
    if count.size == 0 or count.max() < 0:
        return -1, 0
    h = int(np.argmax(count))                                # the first maximum
    c = int(count[h])
    return (h if c >= min_inliers else -1), c


def moments_np(q, frame_id, winner, o):
    """ step 5: the ten sums (int64) over the inliers of hypothesis `winner`; zero without a winner """
    sums = np.zeros(10, np.int64)
    if winner < 0:
        return sums
    n, d0, nn, _ = planes_np(q, frame_id, o)
    q64 = q.astype(np.int64)
    inl = _inlier_mask(q64, n[winner:winner + 1], d0[winner:winner + 1], o['tq2'] * nn[winner:winner + 1])[:, 0]
    x, y, z = q64[inl].T
    sums[:] = [x.size, x.sum(), y.sum(), z.sum(), (x * x).sum(), (x * z).sum(), (z * z).sum(), (x * y).sum(), (z * y).sum(), (y * y).sum()]
    return sums


# ---------------------------------------------------------------------------------------------------- step 6, host only
def solve_moments(sums):
    """ the ten integer sums of one frame -> (plane (4,) float64, rms in metres), or (None, nan) when there is no plane.  Regression of y
    on (x, z): the centred moments, the 2 x 2 determinant and the numerators are exact Python integers (cxx = Sxx N - Sx^2 ...), each
    ratio is rounded to float64 once.  det <= 0 (fewer than three inliers, or all on one vertical line): no plane.  The plane is
    (a, -1, c, d) / sqrt(a^2 + 1 + c^2) with d in metres: unit normal, pointing up, canonical_plane's convention.  rms: the root mean
    square distance of the inliers from the plane, from the same sums. """
    N, Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, Szy, Syy = [int(v) for v in sums]
    if N < 3:
        return None, float('nan')
    cxx, cxz, czz = Sxx * N - Sx * Sx, Sxz * N - Sx * Sz, Szz * N - Sz * Sz
    cxy, czy, cyy = Sxy * N - Sx * Sy, Szy * N - Sz * Sy, Syy * N - Sy * Sy
    det = cxx * czz - cxz * cxz
    if det <= 0:
        return None, float('nan')
    na, nc = cxy * czz - czy * cxz, czy * cxx - cxy * cxz
    a, c = float(Fraction(na, det)), float(Fraction(nc, det))
    d = float(Fraction(Sy * det - na * Sx - nc * Sz, det * N * Q))
    sse = Fraction(cyy * det - na * cxy - nc * czy, det * N * N)           # mean squared residual in y, quanta^2 (>= 0 up to nothing: exact)
    norm = math.sqrt(a * a + 1.0 + c * c)
    rms = math.sqrt(max(0.0, float(sse))) / Q / norm
    return np.array([a, -1.0, c, d], np.float64) / norm, rms


def _assemble(kept, winner, inliers, sums):
    F = len(kept)
    planes = np.full((F, 4), np.nan, np.float64)
    rms = np.full(F, np.nan, np.float64)
    valid = np.zeros(F, bool)
    for f in range(F):
        if winner[f] >= 0:
            plane, r = solve_moments(sums[f])
            if plane is not None:
                planes[f], rms[f], valid[f] = plane, r, True
    return {'planes': planes, 'valid': valid, 'kept': np.asarray(kept, np.int32), 'winner': np.asarray(winner, np.int32),
            'inliers': np.asarray(inliers, np.int32), 'sums': np.asarray(sums, np.int64).reshape(F, 10), 'rms': rms}


def _check_frames(points_list, T_list, frame_ids):
    if not (len(points_list) == len(T_list) == len(frame_ids)):
        raise ValueError('{} scans, {} matrices and {} frame ids'.format(len(points_list), len(T_list), len(frame_ids)))
    pts = [np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 4)) for p in points_list]
    Ts = [np.asarray(T, np.float64).reshape(3, 4) for T in T_list]
    for p in pts:
        if p.shape[0] > MAX_POINTS:
            raise ValueError('a scan of {} points: a frame takes up to {}'.format(p.shape[0], MAX_POINTS))
    ids = [int(v) for v in frame_ids]
    if any(not 0 <= v < (1 << 32) for v in ids):
        raise ValueError('frame ids are uint32')
    return pts, Ts, ids


# ---------------------------------------------------------------------------------------------------- the two forms
def fit_np(points_list, T_list, frame_ids, **options):
    """ the fit in NumPy: per frame the (n, 4) float32 scan, the (3, 4) float64 matrix velodyne -> rectified camera and the uint32 frame id
    -> dict: planes (F, 4) float64 (NaN rows where invalid), valid (F,) bool, kept, winner, inliers (F,) int32, sums (F, 10) int64,
    rms (F,) float64.  Options: DEFAULTS. """
    o = resolve_options(**options)
    pts, Ts, ids = _check_frames(points_list, T_list, frame_ids)
    kept, winner, inliers, sums = [], [], [], []
    for p, T, fid in zip(pts, Ts, ids):
        q = quantise_np(p, T, o['region_q'])
        w, c = winner_np(score_np(q, fid, o), o['min_inliers'])
        kept.append(q.shape[0]); winner.append(w); inliers.append(c); sums.append(moments_np(q, fid, w, o))
    return _assemble(kept, winner, inliers, np.asarray(sums, np.int64).reshape(len(pts), 10))


def device_stages(points_list, T_list, frame_ids, **options):
    """ the four launches on the current device, everything fetched: dict q (total, 3) int32 (a frame's kept points at the head of its own
    segment, zeros behind), offsets (F + 1,), kept (F,), count (F, H), winner, inliers (F,) int32, sums (F, 10) int64.  What fit_device
    is made of; the tests compare every stage.  Raises GppError without a GPU. """
    import torch
    from ..backend import hip
    dev = hip.require_device()
    o = resolve_options(**options)
    pts, Ts, ids = _check_frames(points_list, T_list, frame_ids)
    F = len(pts)
    if F > MAX_FRAMES:
        raise ValueError('{} frames in one call: the device form takes up to {} (fit_pool chunks a dataset)'.format(F, MAX_FRAMES))
    sizes = [p.shape[0] for p in pts]
    offsets = np.zeros(F + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    total, max_points = int(offsets[-1]), max(sizes + [0])
    if total > (1 << 30):
        raise ValueError('{} points in one call: the device form takes up to 2^30'.format(total))
    up = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
    points_d = up(np.concatenate(pts + [np.zeros((0, 4), np.float32)]))
    offsets_d = up(offsets.astype(np.int32))
    T_d = up(np.asarray(Ts, np.float64).reshape(F, 12))
    ids_d = up(np.asarray(ids, np.uint32).view(np.int32))
    q, kept = hip.road_points(points_d, offsets_d, T_d, max_points, o['region_q'])
    count = hip.road_score(q, offsets_d, kept, ids_d, o['seed'], max_points, o['H'], o['c2'], o['hlo2'], o['hhi2'], o['tq2'])
    winner, inliers = hip.road_winner(count, o['min_inliers'])
    sums = hip.road_moments(q, offsets_d, kept, ids_d, o['seed'], winner, max_points, o['H'], o['tq2'])
    torch.cuda.synchronize(dev)
    return {'q': q.cpu().numpy(), 'offsets': offsets.astype(np.int32), 'kept': kept.cpu().numpy(), 'count': count.cpu().numpy(),
            'winner': winner.cpu().numpy(), 'inliers': inliers.cpu().numpy(), 'sums': sums.cpu().numpy()}


def fit_device(points_list, T_list, frame_ids, **options):
    """ fit_np's dict from the device: gpp_road_points_i32, gpp_road_score, gpp_road_winner and gpp_road_moments on one chunk of frames,
    one fetch, then solve_moments per frame.  Raises GppError without a GPU. """
    s = device_stages(points_list, T_list, frame_ids, **options)
    return _assemble(s['kept'], s['winner'], s['inliers'], s['sums'])


# ---------------------------------------------------------------------------------------------------- several planes per frame (4.24)
def round_seed(seed, r):
    """ the seed of round r: (seed + r * ROUND_SEED_STEP) mod 2^32 """
    return (int(seed) + int(r) * ROUND_SEED_STEP) & 0xffffffff


def peel_np(q, frame_id, winner, o):
    """ the peel of one frame: the points of q (m, 3) int32 that are NOT inliers of hypothesis `winner` under o['seed'], in their order.
    No winner (< 0 or >= H): the frame is finished, (0, 3).  The inlier rule is gpp_road_moments': a winner whose plane has nn = 0, or a
    frame of fewer than three points (hand-set winners only), has no inliers and every point stays. """
    q = np.asarray(q, np.int32).reshape(-1, 3)
    if winner < 0 or winner >= o['H']:
        return q[:0].copy()
    n, d0, nn, _ = planes_np(q, frame_id, o)
    if not nn[winner] > 0.0:
        return q.copy()
    inl = _inlier_mask(q.astype(np.int64), n[winner:winner + 1], d0[winner:winner + 1], o['tq2'] * nn[winner:winner + 1])[:, 0]
    return np.ascontiguousarray(q[~inl])


def _check_rounds(planes_per_frame, min_share):
    P = int(planes_per_frame)
    if P != planes_per_frame or P < 1 or P > 16:
        raise ValueError('planes_per_frame {}: needs a whole number 1 .. 16'.format(planes_per_frame))
    share = float(min_share)
    if not 0.0 <= share <= 1.0:
        raise ValueError('min_share {}: needs 0 .. 1'.format(min_share))
    return P, share


def _assemble_rounds(kept, winner, inliers, sums, min_share):
    """ the host's step of section 4.24 on (F, P) stages: round r of a frame is valid iff every earlier round is, it has a winner,
    solve_moments gives a plane and, for r >= 1, inliers_r >= ceil(min_share * kept_0), exactly (Fraction of the float64 min_share) """
    kept, winner, inliers = [np.asarray(v, np.int32) for v in (kept, winner, inliers)]
    F, P = kept.shape
    sums = np.asarray(sums, np.int64).reshape(F, P, 10)
    planes = np.full((F, P, 4), np.nan, np.float64)
    rms = np.full((F, P), np.nan, np.float64)
    valid = np.zeros((F, P), bool)
    share = Fraction(float(min_share))
    for f in range(F):
        need = math.ceil(share * int(kept[f, 0]))
        for r in range(P):
            if winner[f, r] < 0 or (r >= 1 and int(inliers[f, r]) < need):
                break
            plane, v = solve_moments(sums[f, r])
            if plane is None:
                break
            planes[f, r], rms[f, r], valid[f, r] = plane, v, True
    return {'planes': planes, 'valid': valid, 'kept': kept, 'winner': winner, 'inliers': inliers, 'sums': sums, 'rms': rms}


def np_round_stages(points_list, T_list, frame_ids, planes_per_frame, **options):
    """ every stage of every round in NumPy: a list of P dicts q (list of (m, 3) int32 per frame), kept, count (F, H), winner, inliers,
    sums (F, 10).  What fit_rounds_np is made of """
    o = resolve_options(**options)
    P, _ = _check_rounds(planes_per_frame, 0.0)
    pts, Ts, ids = _check_frames(points_list, T_list, frame_ids)
    q = [quantise_np(p, T, o['region_q']) for p, T in zip(pts, Ts)]
    rounds = []
    for r in range(P):
        orr = dict(o, seed=round_seed(o['seed'], r))
        count = [score_np(v, fid, orr) for v, fid in zip(q, ids)]
        picks = [winner_np(c, o['min_inliers']) for c in count]
        sums = [moments_np(v, fid, w, orr) for v, fid, (w, _) in zip(q, ids, picks)]
        rounds.append({'q': q, 'kept': np.asarray([v.shape[0] for v in q], np.int32), 'count': np.asarray(count, np.int32).reshape(len(q), o['H']),
                       'winner': np.asarray([w for w, _ in picks], np.int32), 'inliers': np.asarray([c for _, c in picks], np.int32),
                       'sums': np.asarray(sums, np.int64).reshape(len(q), 10)})
        if r + 1 < P:
            q = [peel_np(v, fid, w, orr) for v, fid, (w, _) in zip(q, ids, picks)]
    return rounds


def _stack_rounds(rounds, min_share):
    stack = lambda key: np.stack([r[key] for r in rounds], axis=1)  # noqa: E731
    return _assemble_rounds(stack('kept'), stack('winner'), stack('inliers'), stack('sums'), min_share)


def fit_rounds_np(points_list, T_list, frame_ids, planes_per_frame, min_share=MIN_SHARE, **options):
    """ up to planes_per_frame planes per frame in NumPy (section 4.24): fit_np's dict with a round axis -- planes (F, P, 4) float64 (NaN
    where invalid), valid (F, P) bool, kept, winner, inliers (F, P) int32, sums (F, P, 10) int64, rms (F, P) float64.  Round 0 is fit_np.
    Options: DEFAULTS. """
    P, share = _check_rounds(planes_per_frame, min_share)
    return _stack_rounds(np_round_stages(points_list, T_list, frame_ids, P, **options), share)


def _device_rounds(points_list, T_list, frame_ids, P, everything, **options):
    import torch
    from ..backend import hip
    dev = hip.require_device()
    o = resolve_options(**options)
    pts, Ts, ids = _check_frames(points_list, T_list, frame_ids)
    F = len(pts)
    if F > MAX_FRAMES:
        raise ValueError('{} frames in one call: the device form takes up to {} (fit_pool chunks a dataset)'.format(F, MAX_FRAMES))
    sizes = [p.shape[0] for p in pts]
    offsets = np.zeros(F + 1, np.int64)
    offsets[1:] = np.cumsum(sizes)
    total, max_points = int(offsets[-1]), max(sizes + [0])
    if total > (1 << 30):
        raise ValueError('{} points in one call: the device form takes up to 2^30'.format(total))
    up = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
    points_d = up(np.concatenate(pts + [np.zeros((0, 4), np.float32)]))
    offsets_d = up(offsets.astype(np.int32))
    T_d = up(np.asarray(Ts, np.float64).reshape(F, 12))
    ids_d = up(np.asarray(ids, np.uint32).view(np.int32))
    q, kept = hip.road_points(points_d, offsets_d, T_d, max_points, o['region_q'])
    held = []
    for r in range(P):
        seed = round_seed(o['seed'], r)
        count = hip.road_score(q, offsets_d, kept, ids_d, seed, max_points, o['H'], o['c2'], o['hlo2'], o['hhi2'], o['tq2'])
        winner, inliers = hip.road_winner(count, o['min_inliers'])
        sums = hip.road_moments(q, offsets_d, kept, ids_d, seed, winner, max_points, o['H'], o['tq2'])
        held.append({'q': q, 'kept': kept, 'count': count, 'winner': winner, 'inliers': inliers, 'sums': sums} if everything else
                    {'kept': kept, 'winner': winner, 'inliers': inliers, 'sums': sums})
        if r + 1 < P:                                         # (without `everything` the buffer of two rounds ago is free again: two in use)
            q, kept = hip.road_peel(q, offsets_d, kept, ids_d, seed, winner, max_points, o['H'], o['tq2'])
    torch.cuda.synchronize(dev)
    return [dict({k: v.cpu().numpy() for k, v in h.items()}, offsets=offsets.astype(np.int32)) for h in held]


def device_round_stages(points_list, T_list, frame_ids, planes_per_frame, **options):
    """ device_stages per round: a list of P dicts q (total, 3) int32 (a frame's points of that round at the head of its own segment,
    zeros behind), offsets (F + 1,), kept (F,), count (F, H), winner, inliers (F,) int32, sums (F, 10) int64 -- gpp_road_points_i32 once,
    then per round score, winner and moments under the round's seed, and gpp_road_peel_i32 between two rounds.  What fit_rounds_device is
    made of; the tests compare every stage.  Raises GppError without a GPU. """
    P, _ = _check_rounds(planes_per_frame, 0.0)
    return _device_rounds(points_list, T_list, frame_ids, P, True, **options)


def fit_rounds_device(points_list, T_list, frame_ids, planes_per_frame, min_share=MIN_SHARE, **options):
    """ fit_rounds_np's dict from the device: equal to it entry for entry, planes bit for bit.  Raises GppError without a GPU. """
    P, share = _check_rounds(planes_per_frame, min_share)
    return _stack_rounds(_device_rounds(points_list, T_list, frame_ids, P, False, **options), share)


# ---------------------------------------------------------------------------------------------------- files
def read_velodyne(path):
    """ a KITTI velodyne .bin: (n, 4) float32 x y z reflectance """
    raw = np.fromfile(path, dtype=np.float32)
    if raw.size % 4:
        raise ValueError('{}: {} float32 values are no whole number of (x, y, z, reflectance) points'.format(path, raw.size))
    return raw.reshape(-1, 4)


def read_velo_calibration(path):
    """ R0_rect . Tr_velo_to_cam of a KITTI calibration file as (3, 4) float64: a velodyne point (x, y, z, 1) -> rectified camera metres """
    with open(path, 'r') as f:
        lines = f.readlines()

    def numbers(key, count):
        line = ([v for v in lines if v.startswith(key + ':')] or [''])[0]
        values = line.split(':', 1)[-1].split()
        if len(values) != count:
            raise ValueError('{}: no {} line with {} numbers'.format(path, key, count))
        return np.array([float(v) for v in values], np.float64)
    R0 = numbers('R0_rect', 9).reshape(3, 3)
    Tr = numbers('Tr_velo_to_cam', 12).reshape(3, 4)
    return R0 @ Tr


def read_plane_files(directory):
    """ the planes/NNNNNN.txt files that KITTI-derived sets distribute (a few header lines, then one line of four numbers a b c d in camera
    coordinates), sorted by name -> (pool (N, 4) float64, file names): a second way to a pool for plane_db.distil """
    files = sorted(f for f in os.listdir(directory) if f.endswith('.txt'))
    rows = []
    for name in files:
        path = os.path.join(directory, name)
        row = None
        with open(path, 'r') as f:
            for line in f:
                parts = line.split()
                if len(parts) == 4:
                    try:
                        row = [float(v) for v in parts]
                    except ValueError:
                        continue
        if row is None or not all(math.isfinite(v) for v in row):
            raise ValueError('{}: no line of four numbers'.format(path))
        rows.append(row)
    if not rows:
        raise ValueError('{}: no plane files'.format(directory))
    return np.asarray(rows, np.float64).reshape(-1, 4), files


def _chunks(sizes, H, chunk_frames, budget, point_bytes=28):
    """ consecutive index ranges: at most chunk_frames frames and about `budget` device bytes (28 per point, 4 H per frame) each; with
    several planes per frame the peel's second point buffer makes it 40 per point """
    out, at, n, used = [], 0, 0, 0
    for i, s in enumerate(sizes):
        need = point_bytes * s + 4 * H + 256
        if n and (n >= chunk_frames or used + need > budget):
            out.append((at, i))
            at, n, used = i, 0, 0
        n, used = n + 1, used + need
    if n:
        out.append((at, len(sizes)))
    return out


def fit_pool(velodyne_dir, calib_dir, device=True, chunk_frames=64, chunk_bytes=CHUNK_BYTES, planes_per_frame=1, min_share=MIN_SHARE,
             **options):
    """ the pool of a dataset: the .bin scans of `velodyne_dir` sorted by name (frame_id = the position in that list), the calibration files
    of the same stems in `calib_dir` -> dict: planes (V, 4) float64, the valid frames' planes in file order; files, their names; frames,
    every scan's name; record, fit_np's dict over all frames.  Frames are read and fitted in chunks of up to chunk_frames frames and about
    chunk_bytes device bytes; a frame's result does not depend on the chunking.  device=False: fit_np instead of fit_device.
    planes_per_frame > 1 (section 4.24): fit_rounds_device / fit_rounds_np -- planes (V, 4), the valid planes in frame order and within a
    frame in round order; files, the scan's name once per plane; rounds (V,) int32, each plane's round; record, the rounds dict. """
    files = sorted(f for f in os.listdir(velodyne_dir) if f.endswith('.bin'))
    if not files:
        raise ValueError('{}: no .bin scans'.format(velodyne_dir))
    resolve_options(**options)
    P, share = _check_rounds(planes_per_frame, min_share)
    sizes = [os.path.getsize(os.path.join(velodyne_dir, f)) // 16 for f in files]
    H = int(dict(DEFAULTS, **options)['hypotheses'])
    if P == 1:
        fit = fit_device if device else fit_np
    else:
        one = fit_rounds_device if device else fit_rounds_np
        fit = lambda pts, Ts, ids, **kw: one(pts, Ts, ids, P, share, **kw)  # noqa: E731
    parts = []
    for a, b in _chunks(sizes, H, max(1, min(int(chunk_frames), MAX_FRAMES)), int(chunk_bytes), 28 if P == 1 else 40):
        pts = [read_velodyne(os.path.join(velodyne_dir, f)) for f in files[a:b]]
        Ts = [read_velo_calibration(os.path.join(calib_dir, os.path.splitext(f)[0] + '.txt')) for f in files[a:b]]
        parts.append(fit(pts, Ts, list(range(a, b)), **options))
    record = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    valid = record['valid']
    if P == 1:
        return {'planes': np.ascontiguousarray(record['planes'][valid]), 'files': [f for f, v in zip(files, valid) if v], 'frames': files,
                'record': record}
    at, rounds = np.nonzero(valid)                            # row-major: frame order, within a frame round order
    return {'planes': np.ascontiguousarray(record['planes'][valid]), 'files': [files[f] for f in at], 'rounds': rounds.astype(np.int32),
            'frames': files, 'record': record}
