"""
Smoothing finished tracks offline: a backward Rauch-Tung-Striebel pass over the Kalman filter of utils/track.py, and the filling of
short gaps -- DESIGN.md section 4.35 is the specification, include/gpp.h (gpp_track_smooth_f64) the contract.  The tracker writes
filtered positions: the cuboid at frame k knows nothing of the frames behind it, and a frame in which the detector missed a car stays a
hole in the track file.  Whoever tracks a recorded sequence has all of it in hand: this stage runs section 4.34's filter forward over
every SEGMENT of an identity -- the state (x, z, vx, vz); the row noise, predict, the ground rotation, the update and the birth covariance
are utils/track_kf.py's, the functions the tracker calls -- then backward, and gives every detected row its smoothed x, z and alpha, every missed frame inside a
segment a FILL row between its two detected neighbours, and both the position block of the smoothed covariance.

    segments_of      ids (N, D) -> the index: segments, their cells, a row or a gap per cell (NumPy, on the host)
    smooth_np        NumPy, no GPU and no library: all segments at once, cell by cell; one NumPy operation per float64 operation of the
                     rule, no BLAS and no np.linalg
    smooth_device    csrc/track_smooth.hip: two launches on the current stream, tensors in and out
    merge_fills      per frame the rows, ids and hits with the fills appended, ready for utils.track.tracking_lines

The noise is utils.track.check_noise's dict; there are no defaults for it and none for max_gap.
"""
import collections

import numpy as np

from . import track as T
from . import track_kf as KF

POSE_COLS = T.POSE_COLS
CODE_COLS = (13, 14, 33, 34, 35)            # gpp_pose_f32's row: label, orientation class, padding -- codes, not measures: never interpolated
SET_COLS = (19, 21, 25, 32)                 # what a fill computes: x_s, z_s, alpha, r_y
PI = T.PI

Index = collections.namedtuple('Index', 'seg_start seg_frame cell_row seg_id max_gap')
Index.__doc__ = """ the segments of a finished run: seg_start (n_seg + 1) int64 -- segment s owns the cells [seg_start[s], seg_start[s + 1]) --,
seg_frame (n_seg) int32 -- the frame of its first cell; cell c is frame seg_frame[s] + c --, cell_row (cells) int32 -- the flat row index
frame * D + d of the cell's detection, -1 for a gap --, seg_id (n_seg) int32 -- the identity --, max_gap """


def segments_of(ids, seq_start, max_gap, rows=None):
    """ ids (N, D) int32 (-1: no identity; a device tensor is copied back), seq_start (S + 1,) ascending frame offsets (None: one sequence
    of all frames), max_gap = G >= 0 -> the Index.  A segment is a maximal run of one id's rows in one sequence whose consecutive
    detections lie at most G + 1 frames apart; a longer gap ends it, and the next detection starts a new one under the same id.  rows
    (N, D, 36), when given: a row with a NaN in column 19 or 21 has no cell.  Frames outside every sequence have none either.  The
    segments come ordered by (sequence, id, first frame).  ValueError: an id twice in one frame """
    if hasattr(ids, 'cpu'):
        ids = ids.cpu().numpy()
    if hasattr(rows, 'cpu'):
        rows = rows.cpu().numpy()
    ids = np.asarray(ids)
    if ids.ndim != 2:
        raise ValueError('segments_of: ids must be (N, D), got {}'.format(ids.shape))
    if int(max_gap) != max_gap or max_gap < 0:
        raise ValueError('segments_of: max_gap must be an integer >= 0, got {!r}'.format(max_gap))
    G, (N, D) = int(max_gap), ids.shape
    seq_start = np.array([0, N] if seq_start is None else seq_start, np.int64).reshape(-1)
    if seq_start.size < 1 or (np.diff(seq_start) < 0).any() or seq_start[0] < 0 or seq_start[-1] > N:
        raise ValueError('segments_of: seq_start must ascend inside [0, {}], got {}'.format(N, seq_start.tolist()))
    keep = ids >= 0
    if rows is not None:
        rows = np.asarray(rows)
        if rows.shape != (N, D, POSE_COLS):
            raise ValueError('segments_of: rows must be ({}, {}, {}), got {}'.format(N, D, POSE_COLS, rows.shape))
        keep &= ~(np.isnan(rows[..., 19]) | np.isnan(rows[..., 21]))
    frame = np.broadcast_to(np.arange(N)[:, None], (N, D))
    keep &= (frame >= seq_start[0]) & (frame < seq_start[-1])
    flat = np.flatnonzero(keep)
    f, who = flat // max(D, 1), ids.reshape(-1)[flat].astype(np.int64)
    seq = np.searchsorted(seq_start, f, side='right') - 1
    order = np.lexsort((f, who, seq))
    flat, f, who, seq = flat[order], f[order], who[order], seq[order]
    same = (seq[1:] == seq[:-1]) & (who[1:] == who[:-1])
    if (same & (f[1:] == f[:-1])).any():
        k = int(np.flatnonzero(same & (f[1:] == f[:-1]))[0])
        raise ValueError('segments_of: the id {} stands twice in frame {}'.format(int(who[k]), int(f[k])))
    first = np.ones(flat.size, bool)
    first[1:] = ~(same & (f[1:] - f[:-1] <= G + 1))
    seg = np.cumsum(first) - 1                                            # the segment of every detection
    heads = np.flatnonzero(first)
    last = np.append(heads[1:], flat.size)[:heads.size] - 1             # (no detection at all: no segment)
    length = f[last] - f[heads] + 1
    seg_start = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    cell_row = np.full(int(seg_start[-1]), -1, np.int32)
    cell_row[seg_start[seg] + (f - f[heads][seg])] = flat
    return Index(seg_start, f[heads].astype(np.int32), cell_row, who[heads].astype(np.int32), G)


def reorder(index, order):
    """ the same segments in another order (a permutation of range(n_seg)): what no output of the smoother depends on, save the fills'
    own order, which is the cells' """
    order = np.asarray(order, np.int64)
    lo, hi = index.seg_start[:-1][order], index.seg_start[1:][order]
    cells = np.concatenate([index.cell_row[a:b] for a, b in zip(lo, hi)] + [np.zeros(0, np.int32)])
    return Index(np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64), index.seg_frame[order], cells.astype(np.int32),
                 index.seg_id[order], index.max_gap)


def check_index(index, N, D):
    """ what gpp_track_smooth_f64 refuses with GPP_ERR_BAD_ARG, as a ValueError: -> (seg_start, seg_frame, cell_row) as it takes them """
    seg_start, seg_frame = np.ascontiguousarray(index.seg_start, np.int64), np.ascontiguousarray(index.seg_frame, np.int32)
    cell_row = np.ascontiguousarray(index.cell_row, np.int32)
    n = seg_frame.size
    if seg_start.shape != (n + 1,) or seg_start[0] != 0 or (np.diff(seg_start) <= 0).any() or seg_start[-1] != cell_row.size:
        raise ValueError('track_smooth: seg_start must ascend strictly from 0 to the number of cells')
    if D > T.MAX_DETECTIONS:
        raise ValueError('track_smooth: {} rows in a frame, at most {}'.format(D, T.MAX_DETECTIONS))
    length = np.diff(seg_start)
    if n and ((seg_frame < 0).any() or (seg_frame + length > N).any()):
        raise ValueError('track_smooth: a segment leaves the frames [0, {})'.format(N))
    if n and ((cell_row[seg_start[:-1]] < 0).any() or (cell_row[seg_start[1:] - 1] < 0).any()):
        raise ValueError("track_smooth: a segment's first and last cell must be detections")
    frame = np.repeat(seg_frame.astype(np.int64), length) + (np.arange(cell_row.size) - np.repeat(seg_start[:-1], length))
    det = cell_row >= 0
    if (cell_row < -1).any() or (cell_row[det] >= N * D).any() or (cell_row[det] // max(D, 1) != frame[det]).any():
        raise ValueError("track_smooth: a cell's row must lie in the cell's own frame")
    if np.unique(cell_row[det]).size != int(det.sum()):
        raise ValueError('track_smooth: a row stands in two cells')
    return seg_start, seg_frame, cell_row


def mul(X, Y):
    """ section 4.35: the product of two general 2 x 2 blocks (xx, xz, zx, zz), every multiply and every add separate """
    return ((X[0] * Y[0]) + (X[1] * Y[2]), (X[0] * Y[1]) + (X[1] * Y[3]), (X[2] * Y[0]) + (X[3] * Y[2]), (X[2] * Y[1]) + (X[3] * Y[3]))


def tr(X):
    return (X[0], X[2], X[1], X[3])


def add(X, Y):
    return tuple(x + y for x, y in zip(X, Y))


def sub(X, Y):
    return tuple(x - y for x, y in zip(X, Y))


def sym(xx, xz, zz):
    return (xx, xz, xz, zz)


def predict(s, q_pos, q_vel):
    """ section 4.34, 1 predict, on the 14 words x z vx vz Axx Axz Azz Bxx Bxz Bzx Bzz Cxx Cxz Czz (a list of arrays over the segments) """
    return [s[0] + s[2], s[1] + s[3], s[2], s[3]] + KF.predict_cov(s[4:], q_pos, q_vel)


def ego_step(s, g, t0, t2):
    """ section 4.35, the ego step: the mean by the ground part only, the covariance as section 4.34's 1b; g = (g00, g01, g10, g11) """
    x, z, vx, vz = s[:4]
    return [((g[0] * x) + (g[1] * z)) + t0, ((g[2] * x) + (g[3] * z)) + t2, (g[0] * vx) + (g[1] * vz), (g[2] * vx) + (g[3] * vz)] + KF.turn_cov(s[4:], g)


def born(x, z, R, speed):
    """ section 4.34, 7 births: mean (x, z, 0, 0), A = R of the row, B = 0, C = birth_speed^2 I """
    zero = np.zeros_like(x)
    return [x, z, zero, zero] + KF.born_cov(R, speed)


def update(s, xr, zr, R):
    """ section 4.34, 5 update -> (the 14 words, det > 0); where det is not > 0 the words are not to be used: the caller restarts """
    mean, P, good = KF.update(s[:4], s[4:], R, xr - s[0], zr - s[1])
    return mean + P, good


def smooth_step(sm, pp, pf, g):
    """ section 4.35, one backward step: sm the smoothed words of cell c + 1, pp the predicted ones of c + 1, pf the filtered ones of c, g
    the ground rotation of the transition (None: no records) -> (the smoothed words of c, whether both determinants were > 0); where
    they were not the words are not to be used: the step is skipped """
    A, B = sym(pp[4], pp[5], pp[6]), tuple(pp[7:11])
    dA = (A[0] * A[3]) - (A[1] * A[1])
    iA = sym(A[3] / dA, -(A[1] / dA), A[0] / dA)
    W = mul(iA, B)
    Tm = mul(tr(B), W)
    sxx, sxz, szz = pp[11] - Tm[0], pp[12] - Tm[1], pp[13] - Tm[3]
    dS = (sxx * szz) - (sxz * sxz)
    iS = sym(szz / dS, -(sxz / dS), sxx / dS)
    Fm = tuple(-v for v in mul(W, iS))
    E = sub(iA, mul(Fm, tr(W)))
    fA, fB, fC = sym(pf[4], pf[5], pf[6]), tuple(pf[7:11]), sym(pf[11], pf[12], pf[13])
    U1, U2, U3, U4 = add(fA, fB), fB, add(tr(fB), fC), fC
    if g is not None:
        gt = tr(g)
        U1, U2, U3, U4 = mul(U1, gt), mul(U2, gt), mul(U3, gt), mul(U4, gt)
    J1, J2 = add(mul(U1, E), mul(U2, tr(Fm))), add(mul(U1, Fm), mul(U2, iS))
    J3, J4 = add(mul(U3, E), mul(U4, tr(Fm))), add(mul(U3, Fm), mul(U4, iS))
    dpx, dpz, dvx, dvz = sm[0] - pp[0], sm[1] - pp[1], sm[2] - pp[2], sm[3] - pp[3]
    DA, DB = sym(sm[4] - pp[4], sm[5] - pp[5], sm[6] - pp[6]), tuple(sm[k] - pp[k] for k in range(7, 11))
    DC = sym(sm[11] - pp[11], sm[12] - pp[12], sm[13] - pp[13])
    N1, N2 = add(mul(J1, DA), mul(J2, tr(DB))), add(mul(J1, DB), mul(J2, DC))
    N3, N4 = add(mul(J3, DA), mul(J4, tr(DB))), add(mul(J3, DB), mul(J4, DC))
    QA, QB = add(mul(N1, tr(J1)), mul(N2, tr(J2))), add(mul(N1, tr(J3)), mul(N2, tr(J4)))
    QC = add(mul(N3, tr(J3)), mul(N4, tr(J4)))
    new = [pf[0] + (((J1[0] * dpx) + (J1[1] * dpz)) + ((J2[0] * dvx) + (J2[1] * dvz))),
           pf[1] + (((J1[2] * dpx) + (J1[3] * dpz)) + ((J2[2] * dvx) + (J2[3] * dvz))),
           pf[2] + (((J3[0] * dpx) + (J3[1] * dpz)) + ((J4[0] * dvx) + (J4[1] * dvz))),
           pf[3] + (((J3[2] * dpx) + (J3[3] * dpz)) + ((J4[2] * dvx) + (J4[3] * dvz))),
           fA[0] + QA[0], fA[1] + QA[1], fA[3] + QA[3], fB[0] + QB[0], fB[1] + QB[1], fB[2] + QB[2], fB[3] + QB[3],
           fC[0] + QC[0], fC[1] + QC[1], fC[3] + QC[3]]
    return new, (dA > 0.0) & (dS > 0.0)


def smooth_cells(rows, index, noise, ego=None, keep=None):
    """ the two passes over every segment of two or more cells -> table (5, cells) float64: x_s z_s Axx Axz Azz per cell (zeros for a
    segment of one cell).  rows (N, D, 36) float32; keep: a dict that receives 'predicted', 'filtered' and 'smoothed' (14, cells) """
    noise = T.check_noise(noise)
    N, D = rows.shape[:2]
    seg_start, seg_frame, cell_row = check_index(index, N, D)
    if ego is not None:
        ego = T.check_ego(ego, N)
    flat = np.ascontiguousarray(rows, np.float32).reshape(-1, POSE_COLS)
    cells = cell_row.size
    table = np.zeros((5, cells))
    full = {name: np.zeros((14, cells)) for name in ('predicted', 'filtered', 'smoothed')} if keep is not None else None
    length = np.diff(seg_start)
    lanes = np.flatnonzero(length >= 2)
    lanes = lanes[np.argsort(-length[lanes], kind='stable')]            # longest first: the segments still running are a prefix
    if keep is not None:
        keep.update(full)
    if lanes.size == 0:
        return table
    lo, L, frame = seg_start[lanes], length[lanes], seg_frame[lanes].astype(np.int64)
    q_pos, q_vel = noise['process']
    speed = noise['birth_speed']
    first = flat[cell_row[lo]]
    with np.errstate(all='ignore'):
        cur = born(first[:, 19].astype(np.float64), first[:, 21].astype(np.float64), T.row_noise(first, noise), speed)
        cur = [np.array(v, np.float64) for v in cur]
        pred, filt, restart = [None], [np.stack(cur)], [None]
        for c in range(1, int(L[0])):
            k = int((L > c).sum())
            s = predict([v[:k] for v in cur], q_pos, q_vel)
            if ego is not None:
                e = ego[frame[:k] + c]
                s = ego_step(s, (e[:, 0], e[:, 2], e[:, 6], e[:, 8]), e[:, 9], e[:, 11])
            pred.append(np.stack(s))
            code = cell_row[lo[:k] + c]
            det = code >= 0
            r = flat[np.where(det, code, 0)]
            xr, zr = r[:, 19].astype(np.float64), r[:, 21].astype(np.float64)
            R = T.row_noise(r, noise)
            new, good = update(s, xr, zr, R)
            again = born(xr, zr, R, speed)
            fresh = det & ~good
            s = [np.where(det, np.where(good, n, b), p) for n, b, p in zip(new, again, s)]
            restart.append(fresh)
            filt.append(np.stack(s))
            cur = s
        sm = np.zeros((14, lanes.size))
        for c in range(int(L[0]) - 1, -1, -1):
            k, k1 = int((L > c).sum()), int((L > c + 1).sum())
            sm[:, k1:k] = filt[c][:, k1:k]                               # a segment's last cell: its smoothed state is its filtered one
            if k1:
                g = None
                if ego is not None:
                    e = ego[frame[:k1] + c + 1]
                    g = (e[:, 0], e[:, 2], e[:, 6], e[:, 8])
                new, good = smooth_step(list(sm[:, :k1]), list(pred[c + 1][:, :k1]), list(filt[c][:, :k1]), g)
                good = good & ~restart[c + 1][:k1]
                sm[:, :k1] = np.where(good, np.stack(new), filt[c][:, :k1])
            table[:, lo[:k] + c] = sm[[0, 1, 4, 5, 6], :k]
            if full is not None:
                full['smoothed'][:, lo[:k] + c] = sm[:, :k]
                full['filtered'][:, lo[:k] + c] = filt[c][:, :k]
                if c:
                    full['predicted'][:, lo[:k] + c] = pred[c][:, :k]
    return table


def emit(rows, index, table):
    """ section 4.35's outputs from the cell table -> (rows_out (N, D, 36) float32, row_cov (N, D, 3) float64, fill_rows (fills, 36) float32,
    fill_cov (fills, 3) float64) """
    N, D = rows.shape[:2]
    seg_start, cell_row = np.asarray(index.seg_start, np.int64), np.asarray(index.cell_row, np.int32)
    length = np.diff(seg_start)
    out = np.array(rows, np.float32).reshape(-1, POSE_COLS)
    flat = out.copy()
    row_cov = np.zeros((N * D, 3))
    cell_len = np.repeat(length, length)
    cell_lo = np.repeat(seg_start[:-1], length)
    det = np.flatnonzero((cell_row >= 0) & (cell_len >= 2))
    with np.errstate(all='ignore'):
        r = cell_row[det]
        xs, zs = table[0, det], table[1, det]
        out[r, 19], out[r, 21] = xs.astype(np.float32), zs.astype(np.float32)
        out[r, 25] = T.wrap(flat[r, 32].astype(np.float64) - np.arctan2(xs, zs)).astype(np.float32)
        row_cov[r] = table[2:5, det].T
        gap = np.flatnonzero(cell_row < 0)
        # the detected neighbours before and behind: the last / next detection's cell, carried along the cells
        where = np.arange(cell_row.size)
        before = np.maximum.accumulate(np.where(cell_row >= 0, where, -1))
        behind = np.minimum.accumulate(np.where(cell_row >= 0, where, cell_row.size)[::-1])[::-1]
        j0, j1 = before[gap], behind[gap]
        assert ((j0 >= cell_lo[gap]) & (j1 < cell_lo[gap] + cell_len[gap])).all()
        a, b = flat[cell_row[j0]].astype(np.float64), flat[cell_row[j1]].astype(np.float64)
        w = (gap - j0).astype(np.float64) / (j1 - j0).astype(np.float64)
        fill64 = a + (w[:, None] * (b - a))
        fills = fill64.astype(np.float32)
        fills[:, CODE_COLS] = flat[cell_row[j0]][:, CODE_COLS]
        delta = T.wrap(b[:, 32] - a[:, 32])
        delta = np.where(delta >= PI / 2.0, delta - PI, delta)
        delta = np.where(delta < -(PI / 2.0), delta + PI, delta)
        ry = T.wrap(a[:, 32] + (w * delta))
        xs, zs = table[0, gap], table[1, gap]
        fills[:, 19], fills[:, 21], fills[:, 32] = xs.astype(np.float32), zs.astype(np.float32), ry.astype(np.float32)
        fills[:, 25] = T.wrap(ry - np.arctan2(xs, zs)).astype(np.float32)
    return out.reshape(N, D, POSE_COLS), row_cov.reshape(N, D, 3), fills.reshape(-1, POSE_COLS), np.ascontiguousarray(table[2:5, gap].T)


def smooth_np(rows, index, noise, ego=None, keep=None):
    """ the NumPy form: rows (N, D, 36) float32, the RAW rows of a finished run; index: segments_of's; noise: check_noise's dict; ego: None
    or the (N, 16) records of section 4.33 -> (rows_out, row_cov, fill_rows, fill_cov) as gpp_track_smooth_f64 writes them """
    rows = np.asarray(rows, np.float32)
    if rows.ndim != 3 or rows.shape[2] != POSE_COLS:
        raise ValueError('smooth_np: rows must be (N, D, {}), got {}'.format(POSE_COLS, rows.shape))
    return emit(rows, index, smooth_cells(rows, index, noise, ego, keep))


def kf_params(noise):
    """ check_noise's dict -> backend.hip.TrackKfParams """
    from ..backend import hip
    n = T.check_noise(noise)
    return hip.TrackKfParams(n['radial'][0], n['radial'][1], n['tangential'][0], n['tangential'][1], n['process'][0], n['process'][1],
                             n['birth_speed'], 0)


def smooth_device(rows, index, noise, ego=None, out=None, covariance=True):
    """ csrc/track_smooth.hip on the current stream: rows a dense (N, D, 36) float32 device tensor -> (rows_out, row_cov, fill_rows,
    fill_cov) device tensors (the covariances None for covariance=False); out: where the rows go, `rows` itself allowed.  A NumPy array
    goes to the device and the results come back as arrays.  The index and the records stay on the host """
    import torch
    from ..backend import hip
    kf = kf_params(noise)
    if ego is not None:
        ego = T.check_ego(ego, len(rows))
    if isinstance(rows, torch.Tensor):
        seg_start, seg_frame, cell_row = check_index(index, int(rows.shape[0]), int(rows.shape[1]))
        return hip.track_smooth(rows, seg_start, seg_frame, cell_row, kf, ego=ego, out=out, covariance=covariance)
    host = np.ascontiguousarray(rows, np.float32)
    if host.ndim != 3 or host.shape[2] != POSE_COLS:
        raise ValueError('smooth_device: rows must be (N, D, {}), got {}'.format(POSE_COLS, host.shape))
    seg_start, seg_frame, cell_row = check_index(index, host.shape[0], host.shape[1])
    res = hip.track_smooth(torch.as_tensor(host).to(hip.require_device()), seg_start, seg_frame, cell_row, kf, ego=ego, covariance=covariance)
    return tuple(None if t is None else t.cpu().numpy() for t in res)


def merge_fills(rows_out, ids, hits, index, fill_rows):
    """ per frame the rows, ids and hits with the fills appended: lists of N arrays (D_f, 36) float32, (D_f,) int32, (D_f,) int32, ready for
    utils.track.tracking_lines.  A fill carries its segment's id and the hits of the detection before it """
    rows_out, ids, hits = np.asarray(rows_out, np.float32), np.asarray(ids, np.int32), np.asarray(hits, np.int32)
    fill_rows = np.asarray(fill_rows, np.float32).reshape(-1, POSE_COLS)
    N = rows_out.shape[0]
    length = np.diff(index.seg_start)
    cell = np.arange(index.cell_row.size)
    frame = np.repeat(index.seg_frame.astype(np.int64), length) + (cell - np.repeat(index.seg_start[:-1], length))
    who = np.repeat(index.seg_id, length)
    before = np.maximum.accumulate(np.where(index.cell_row >= 0, cell, -1))
    gap = np.flatnonzero(index.cell_row < 0)
    if gap.size != fill_rows.shape[0]:
        raise ValueError('merge_fills: {} gaps in the index, {} fill rows'.format(gap.size, fill_rows.shape[0]))
    fill_hits = hits.reshape(-1)[index.cell_row[before[gap]]]
    out_rows, out_ids, out_hits = [], [], []
    for f in range(N):
        k = np.flatnonzero(frame[gap] == f)
        out_rows.append(np.concatenate([rows_out[f], fill_rows[k]]))
        out_ids.append(np.concatenate([ids[f], who[gap[k]]]).astype(np.int32))
        out_hits.append(np.concatenate([hits[f], fill_hits[k]]).astype(np.int32))
    return out_rows, out_ids, out_hits


def smooth_tracks(rows, ids, hits, noise, max_gap, seq_start=None, ego=None, host=False):
    """ what the command lines do behind a finished run: rows (N, D, 36) RAW rows, ids and hits (N, D) of the tracker -> merge_fills' three
    lists and the number of fills.  host: the NumPy form instead of the device's """
    rows = np.asarray(rows, np.float32)
    index = segments_of(ids, seq_start, max_gap, rows)
    rows_out, _, fill_rows, _ = (smooth_np if host else smooth_device)(rows, index, noise, ego)
    return merge_fills(rows_out, ids, hits, index, fill_rows) + (int(fill_rows.shape[0]),)


def add_arguments(parser, rts='--rts', max_gap='--max-gap'):
    """ the command lines' two arguments (bin/track_results.py --rts --max-gap, bin/run_network.py --track-rts --track-max-gap) """
    parser.add_argument(rts, dest='rts', action='store_true',
                        help='Smooth the finished tracks offline before they are written: a backward Rauch-Tung-Striebel pass over the '
                             'Kalman filter, and a row for every frame the detector missed inside a track (DESIGN.md section 4.35).  Needs '
                             '--track-noise, --track-process and --track-birth-speed (no defaults), under any metric and either filter.')
    parser.add_argument(max_gap, dest='max_gap', type=int, default=None, metavar='G',
                        help='With {}: gaps of up to G frames are filled, a longer one splits the track into two segments.  Default: the '
                             'run\'s max age -- a track of this tracker never has a longer gap.'.format(rts))


def smoother_arguments(args, smooth, max_age):
    """ add_arguments' values, checked: -> the smoother's noise, or None without the option; args.max_gap is filled in (default: max_age).
    ValueError: the option together with `smooth` (it wants the raw rows), a negative gap, a gap without the option, a missing noise """
    if not args.rts:
        if args.max_gap is not None:
            raise ValueError('the gap argument belongs to the offline smoother')
        return None
    if smooth:
        raise ValueError('the offline smoother wants the raw rows: it does not go with the smoothed rows of the tracker')
    if args.max_gap is None:
        args.max_gap = int(max_age)
    if args.max_gap < 0:
        raise ValueError('the largest gap must be >= 0, got {}'.format(args.max_gap))
    return noise_of(args)


def filter_option(args):
    """ utils.track.filter_option for a command line that has the smoother: the three noise arguments may stand without --track-filter
    kalman when they are the smoother's """
    if args.rts and args.track_filter != 'kalman':
        return {}
    return T.filter_option(args)


def noise_of(args):
    """ the smoother's noise from --track-noise, --track-process and --track-birth-speed; ValueError when one is missing or refused """
    if args.track_noise is None or args.track_process is None or args.track_birth_speed is None:
        raise ValueError('the offline smoother needs --track-noise R0 R1 T0 T1, --track-process QP QV and --track-birth-speed V0 (no defaults)')
    return T.check_noise({'radial': tuple(args.track_noise[:2]), 'tangential': tuple(args.track_noise[2:]),
                          'process': tuple(args.track_process), 'birth_speed': args.track_birth_speed})
