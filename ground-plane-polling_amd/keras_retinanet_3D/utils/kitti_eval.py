"""
KITTI's object benchmark for the project's result rows: AP of the image box, the bird's-eye-view (BEV) box and the 3-D box at
Easy / Moderate / Hard, and AOS, for the class Car (neighbouring class Van) -- DESIGN.md section 4.17 is the specification, a
restatement of the devkit's evaluate_object.cpp.  Parity with the devkit itself is UNPINNED (it is not part of this repository).

Two forms of one computation:
    device=False    NumPy, no GPU and no library: per image the overlaps of all (detection, label) pairs at once, the matching
                    vectorised over (metric, difficulty, threshold) and serial over the labels, as the rules demand.
    device=True     csrc/kitti_eval.hip: the overlaps are launched once per chunk of images and read by both passes
                    (gpp_kitti_overlaps_f64, gpp_kitti_stats_f64); only true-positive scores, counts and similarities come back.
Both end in the same host code (thresholds, precision, AP), fed with per-image results summed in image order.

A detection is a row of gpp_pose_f32 (include/gpp.h): float32, so a result file and the rows it was written from score alike only up
to the two decimals of the text.  A label is a (16,) float64 row: type code, the 14 numeric fields of label_2, zero.
"""
import os

import numpy as np

METRICS = ('image', 'bev', '3d')
DIFFICULTIES = ('easy', 'moderate', 'hard')
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0.0, 1.0, 2.0)
MAX_TRUNCATION = (0.15, 0.30, 0.50)
N_SAMPLE_PTS = 41
TYPE_CODES = {'Car': 0, 'Van': 1, 'DontCare': 2}          # anything else: 3
POSE_COLS = 36
LABEL_COLS = 16
MAX_DETECTIONS = 128                                       # what the device form takes per image (include/gpp.h)
MAX_LABELS = 128
OVERLAP_WORKSPACE_BYTES = 256 << 20                        # the device form cuts the dataset into chunks whose overlaps stay below this
# result-file field k (after the type) -> column of a pose row: truncation and occlusion are not kept
_ROW_OF_FIELD = {3: 25, 4: 26, 5: 27, 6: 28, 7: 29, 8: 30, 9: 17, 10: 18, 11: 19, 12: 31, 13: 21, 14: 32, 15: 12}


# ---------------------------------------------------------------------------------------------------- files
def _read_lines(path, what, names=None):
    """ the lines of a label or result file as (n, 16) rows; `names`: a list that receives the type name of every row (utils/label_prep.py) """
    out = []
    with open(path, 'r') as f:
        for n, line in enumerate(f):
            fields = line.split()
            if not fields:
                continue
            if len(fields) not in (15, 16):
                raise ValueError('{}:{}: a {} line has 15 or 16 fields, got {}'.format(path, n + 1, what, len(fields)))
            row = np.zeros(LABEL_COLS, np.float64)
            row[0] = TYPE_CODES.get(fields[0], 3)
            if names is not None:
                names.append(fields[0])
            row[1:15] = [float(v) for v in fields[1:15]]
            row[15] = float(fields[15]) if len(fields) == 16 else np.nan
            out.append(row)
    return np.array(out, np.float64).reshape(-1, LABEL_COLS)


def read_label_file(path):
    """ label_2 lines -> (n, 16) float64: type code (0 Car, 1 Van, 2 DontCare, 3 other), truncation, occlusion, alpha, box x1 y1 x2 y2,
    h w l, x y z, r_y, 0.  A 16th field (a score) is ignored. """
    rows = _read_lines(path, 'label')
    rows[:, 15] = 0.0
    return rows


def read_result_file(path):
    """ result lines -> (n, 16) float64: as read_label_file, with the score in column 15.  A line without a score (15 fields: a label
    file read as a result) scores 1. """
    rows = _read_lines(path, 'result')
    rows[np.isnan(rows[:, 15]), 15] = 1.0
    return rows


def rows_from_results(results, D=None):
    """ (n, 16) result lines -> (D, 36) float32 pose rows (include/gpp.h, gpp_pose_f32): only the columns of the KITTI line are filled
    (12 score, 25 alpha, 26-29 box, 30 h, 17 w, 18 l, 19 x, 31 y, 21 z, 32 r_y; label and orientation class 0); rows beyond the
    detections are -1 throughout, as the device leaves them.  Lines of another type than Car are dropped: every detection is a Car. """
    results = np.asarray(results, np.float64).reshape(-1, LABEL_COLS)
    results = results[results[:, 0] == 0]
    n = results.shape[0]
    D = n if D is None else int(D)
    if n > D:
        raise ValueError('{} detections do not fit {} rows'.format(n, D))
    rows = np.full((D, POSE_COLS), -1.0, np.float32)
    rows[:n] = 0.0
    for field, col in _ROW_OF_FIELD.items():
        rows[:n, col] = results[:, field]
    return rows


# ---------------------------------------------------------------------------------------------------- one image on the host
def _clip(X, Z, n, ax, az, ex, ez):
    """ one Sutherland-Hodgman step for N polygons at once: X, Z (N, 8), n (N,) vertices, against the edge from (ax, az) along (ex, ez) """
    N = X.shape[0]
    idx = np.arange(N)
    NX, NZ, m = np.zeros_like(X), np.zeros_like(Z), np.zeros(N, np.int64)
    for i in range(int(n.max()) if N else 0):
        active = i < n
        j = np.where(i + 1 == n, 0, i + 1) % 8
        px, pz, qx, qz = X[:, i], Z[:, i], X[idx, j], Z[idx, j]
        dp = ex * (pz - az) - ez * (px - ax)
        dq = ex * (qz - az) - ez * (qx - ax)
        in_p, in_q = dp >= 0.0, dq >= 0.0
        put = active & in_p & (m < 8)
        NX[idx[put], m[put]] = px[put]
        NZ[idx[put], m[put]] = pz[put]
        m = m + put
        put = active & (in_p != in_q) & (m < 8)
        den = dq - dp
        NX[idx[put], m[put]] = ((px * dq - qx * dp)[put]) / den[put]
        NZ[idx[put], m[put]] = ((pz * dq - qz * dp)[put]) / den[put]
        m = m + put
    return NX, NZ, m


def _corners(l, w, tx, tz, ry):
    """ the four corners (+,+) (-,+) (-,-) (+,-) of (l/2, w/2), placed: (N, 4) X and Z """
    c, s, hl, hw = np.cos(ry), np.sin(ry), l / 2.0, w / 2.0
    xs = np.stack([hl, -hl, -hl, hl], axis=1)
    zs = np.stack([hw, hw, -hw, -hw], axis=1)
    return c[:, None] * xs + s[:, None] * zs + tx[:, None], -s[:, None] * xs + c[:, None] * zs + tz[:, None]


def rect_intersections(dl, dw, dtx, dtz, dry, gl, gw, gtx, gtz, gry):
    """ the area of the intersection of N pairs of rotated rectangles in the (X, Z) plane, (N,) float64 each: the d rectangle clipped
    against the four edges of the g rectangle, then the area sum (csrc/rot_iou.h; utils/cuboid_nms.py shares it).  No NaN operand. """
    N = dl.shape[0]
    gX, gZ = _corners(gl, gw, gtx, gtz, gry)
    X, Z = np.zeros((N, 8)), np.zeros((N, 8))
    X[:, :4], Z[:, :4] = _corners(dl, dw, dtx, dtz, dry)
    n = np.full(N, 4, np.int64)
    for e in range(4):
        ax, az = gX[:, e], gZ[:, e]
        X, Z, n = _clip(X, Z, n, ax, az, gX[:, (e + 1) & 3] - ax, gZ[:, (e + 1) & 3] - az)
    twice = np.zeros(N)
    idx = np.arange(N)
    for i in range(int(n.max())):
        j = np.where(i + 1 == n, 0, i + 1) % 8
        twice = twice + np.where(i < n, X[:, i] * Z[idx, j] - X[idx, j] * Z[:, i], 0.0)
    return np.where(n < 3, 0.0, np.abs(twice) / 2.0)


def height_overlaps(dty, dh, gty, gh):
    """ the height term of the 3-D overlap: max(0, min(y_d, y_g) - max(y_d - h_d, y_g - h_g)) """
    lo = np.where(dty - dh > gty - gh, dty - dh, gty - gh)
    hh = np.where(dty < gty, dty, gty) - lo
    return np.where(hh > 0.0, hh, 0.0)


def image_overlaps(rows, labels):
    """ rows (D, 36) float32, labels (A, 16) float64 -> (4, D, A) float64: image IoU, BEV IoU, 3-D IoU, image intersection over the
    detection's area.  Rows that are no detection (column 14 < 0) give 0. """
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    labels = np.asarray(labels, np.float64).reshape(-1, LABEL_COLS)
    D, A = rows.shape[0], labels.shape[0]
    out = np.zeros((4, D, A), np.float64)
    if D * A == 0:
        return out
    r = np.repeat(rows.astype(np.float64), A, axis=0)                    # pair p = d * A + a
    g = np.tile(labels, (D, 1))
    live = r[:, 14] >= 0.0
    with np.errstate(invalid='ignore', divide='ignore'):
        # image
        dx1, dy1, dx2, dy2 = r[:, 26], r[:, 27], r[:, 28], r[:, 29]
        gx1, gy1, gx2, gy2 = g[:, 4], g[:, 5], g[:, 6], g[:, 7]
        bad = np.isnan(r[:, 26:30]).any(axis=1) | np.isnan(g[:, 4:8]).any(axis=1)
        w = np.where(dx2 < gx2, dx2, gx2) - np.where(dx1 > gx1, dx1, gx1)
        h = np.where(dy2 < gy2, dy2, gy2) - np.where(dy1 > gy1, dy1, gy1)
        none = (w <= 0.0) | (h <= 0.0)
        inter = w * h
        area_d = (dx2 - dx1) * (dy2 - dy1)
        area_g = (gx2 - gx1) * (gy2 - gy1)
        o_img = np.where(none, 0.0, inter / (area_d + area_g - inter))
        o_dc = np.where(none, 0.0, inter / area_d)
        o_img[bad], o_dc[bad] = np.nan, np.nan
        # bird's-eye view
        dh, dw, dl, dtx, dty, dtz, dry = r[:, 30], r[:, 17], r[:, 18], r[:, 19], r[:, 31], r[:, 21], r[:, 32]
        gh, gw, gl, gtx, gty, gtz, gry = g[:, 8], g[:, 9], g[:, 10], g[:, 11], g[:, 12], g[:, 13], g[:, 14]
        bad_bev = np.isnan(np.stack([dw, dl, dtx, dtz, dry, gw, gl, gtx, gtz, gry])).any(axis=0)
        ok = np.flatnonzero(live & ~bad_bev)
        inter = np.zeros(D * A)
        if ok.size:
            inter[ok] = rect_intersections(dl[ok], dw[ok], dtx[ok], dtz[ok], dry[ok], gl[ok], gw[ok], gtx[ok], gtz[ok], gry[ok])
        area_d, area_g = dl * dw, gl * gw
        o_bev = inter / (area_d + area_g - inter)
        o_bev[bad_bev] = np.nan
        bad_3d = bad_bev | np.isnan(np.stack([dh, dty, gh, gty])).any(axis=0)
        hh = height_overlaps(dty, dh, gty, gh)
        iv = inter * hh
        o_3d = iv / (area_d * dh + area_g * gh - iv)
        o_3d[bad_3d] = np.nan
    for k, o in enumerate((o_img, o_bev, o_3d, o_dc)):
        out[k] = np.where(live, o, 0.0).reshape(D, A)
    return out


def label_status(labels):
    """ (A, 16) -> status (3, A) int8 per difficulty (0 counts, 1 ignored, -1 skipped) and the DontCare mask (A,) """
    labels = np.asarray(labels, np.float64).reshape(-1, LABEL_COLS)
    kind, trunc, occ = labels[:, 0], labels[:, 1], labels[:, 2]
    height = np.abs(labels[:, 7] - labels[:, 5])
    status = np.full((3, labels.shape[0]), -1, np.int8)
    for d in range(3):
        ignore = (occ > MAX_OCCLUSION[d]) | (trunc > MAX_TRUNCATION[d]) | (height < MIN_HEIGHT[d])
        status[d] = np.where(kind == 0, np.where(ignore, 1, 0), np.where(kind == 1, 1, -1))
    return status, kind == 2


def detection_status(rows):
    """ (D, 36) -> status (3, D) int8 per difficulty: 0 counts, 1 too low, -1 no detection (a padding row; every detection is a Car) """
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    height = np.abs(rows[:, 29].astype(np.float64) - rows[:, 27].astype(np.float64))
    status = np.empty((3, rows.shape[0]), np.int8)
    for d in range(3):
        status[d] = np.where(rows[:, 14] >= 0, np.where(height < MIN_HEIGHT[d], 1, 0), -1)
    return status


def match_image(rows, labels, overlaps, min_overlap, thresholds=None, n_thresholds=None):
    """ the matching of one image for every (metric, difficulty[, threshold]) at once.
    thresholds None (pass 1) -> (tp_scores (3, 3, A) float32, NaN where the label takes no true positive; n_gt (3, 3) int32)
    thresholds (3, 3, T) float32, n_thresholds (3, 3) (pass 2) -> (stats (3, 3, T, 3) int32: tp fp fn; similarity (3, 3, T) float64) """
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    labels = np.asarray(labels, np.float64).reshape(-1, LABEL_COLS)
    if rows.shape[0] == 0:                                   # an image without detections: one padding row keeps the shapes alive
        rows, overlaps = np.full((1, POSE_COLS), -1.0, np.float32), np.zeros((4, 1, labels.shape[0]))
    D, A = rows.shape[0], labels.shape[0]
    compute_fp = thresholds is not None
    T = int(thresholds.shape[2]) if compute_fp else 1
    scores = rows[:, 12]
    lstat, is_dc = label_status(labels)
    ds = np.broadcast_to(detection_status(rows).reshape(1, 3, 1, D), (3, 3, T, D))
    mo = np.asarray(min_overlap, np.float64).reshape(3, 1, 1, 1)
    if compute_fp:
        out = scores.reshape(1, 1, 1, D) < np.asarray(thresholds, np.float32)[..., None]          # float32 against float32
        avail = (ds != -1) & ~out
    else:
        avail = (ds != -1) & np.broadcast_to(scores > -np.inf, (3, 3, T, D))                      # (a NaN score is never "> best")
    avail = np.array(avail)
    tp, fn = np.zeros((3, 3, T), np.int32), np.zeros((3, 3, T), np.int32)
    sim = np.zeros((3, 3, T), np.float64)
    tp_scores = np.full((3, 3, A), np.nan, np.float32)
    with np.errstate(invalid='ignore'):
        for a in range(A):
            ls = lstat[:, a].reshape(1, 3, 1)
            if (ls == -1).all():
                continue
            o = np.broadcast_to(overlaps[:3, :, a].reshape(3, 1, 1, D), (3, 3, T, D))
            valid = avail & (o > mo)
            if compute_fp:
                # the free detection of the largest overlap (the first of equals); a too-low one only when nothing else offers
                v0 = valid & (ds == 0)
                has0 = v0.any(axis=3)
                cand = np.where(has0, np.where(v0, o, -1.0).argmax(axis=3), (valid & (ds == 1)).argmax(axis=3))
            else:
                cand = np.where(valid, scores.reshape(1, 1, 1, D), -np.inf).argmax(axis=3)
            has = valid.any(axis=3) & (ls != -1)
            cand_low = np.take_along_axis(ds, cand[..., None], axis=3)[..., 0] == 1
            is_tp = has & ~((ls == 1) | cand_low)
            fn += ~valid.any(axis=3) & (ls == 0)
            tp += is_tp
            if compute_fp:
                delta = labels[a, 3] - rows[:, 25].astype(np.float64)[cand[0]]
                sim[0] = sim[0] + np.where(is_tp[0], (1.0 + np.cos(delta)) / 2.0, 0.0)
            else:
                tp_scores[:, :, a] = np.where(is_tp[:, :, 0], scores[cand[:, :, 0]], np.nan)
            keep = np.take_along_axis(avail, cand[..., None], axis=3)
            np.put_along_axis(avail, cand[..., None], keep & ~has[..., None], axis=3)
        if not compute_fp:
            n_gt = np.broadcast_to((lstat == 0).sum(axis=1).astype(np.int32).reshape(1, 3), (3, 3))
            return tp_scores, np.array(n_gt)
        left = avail & (ds == 0)
        if is_dc.any():
            in_stuff = (overlaps[3][:, is_dc] > mo[0, 0, 0, 0]).any(axis=1)
            left[0] &= ~in_stuff
        fp = left.sum(axis=3).astype(np.int32)
    stats = np.stack([tp, fp, fn], axis=3)
    off = np.arange(T).reshape(1, 1, T) >= np.asarray(n_thresholds).reshape(3, 3, 1)
    stats[off] = 0
    sim[off] = 0.0
    return stats, sim


# ---------------------------------------------------------------------------------------------------- the dataset level (both forms)
def recall_thresholds(tp_scores, n_gt):
    """ the scores at which the recall passes 0, 1/40, 2/40, ...: at most 41, descending (float32) """
    v = np.sort(np.asarray(tp_scores, np.float32))[::-1]
    out, cur, n_gt = [], 0.0, float(n_gt)
    for i in range(v.size):
        l = (i + 1) / n_gt
        r = (i + 2) / n_gt if i < v.size - 1 else l
        if (r - cur) < (cur - l) and i < v.size - 1:
            continue
        out.append(v[i])
        cur += 1.0 / (N_SAMPLE_PTS - 1.0)
        if len(out) == N_SAMPLE_PTS:
            break
    return np.array(out, np.float32)


def thresholds_of(tp_scores, n_gt):
    """ tp_scores (N, 3, 3, A) of all images in image order, n_gt (3, 3) -> thresholds (3, 3, 41) float32 (zero-padded), n (3, 3) int32 """
    thr = np.zeros((3, 3, N_SAMPLE_PTS), np.float32)
    n = np.zeros((3, 3), np.int32)
    for m in range(3):
        for d in range(3):
            v = tp_scores[:, m, d].ravel()
            t = recall_thresholds(v[~np.isnan(v)], n_gt[m, d]) if n_gt[m, d] > 0 else np.zeros(0, np.float32)
            thr[m, d, :t.size], n[m, d] = t, t.size
    return thr, n


def summarise(stats, similarity, thresholds, n_thresholds):
    """ summed stats (3, 3, 41, 3), similarity (3, 3, 41) -> the result dict of evaluate_kitti """
    def curve(num, den, n):
        p = np.zeros(N_SAMPLE_PTS)
        ok = den[:n] > 0
        p[:n][ok] = num[:n][ok] / den[:n][ok].astype(np.float64)
        return np.maximum.accumulate(p[::-1])[::-1]

    def averages(p):
        return 100.0 * float(np.sum(p[1:])) / 40.0, 100.0 * float(np.sum(p[::4])) / 11.0

    result = {}
    for m, metric in enumerate(METRICS):
        for d, difficulty in enumerate(DIFFICULTIES):
            n = int(n_thresholds[m, d])
            tp, fp, fn = (stats[m, d, :n, k] for k in range(3))
            r40, r11 = averages(curve(tp.astype(np.float64), tp + fp, n))
            result[(metric, difficulty)] = {'ap_r40': r40, 'ap_r11': r11, 'thresholds': thresholds[m, d, :n].copy(),
                                            'tp': tp.copy(), 'fp': fp.copy(), 'fn': fn.copy()}
            if m == 0:
                a40, a11 = averages(curve(similarity[m, d], tp + fp, n))
                result[('aos', difficulty)] = {'aos_r40': a40, 'aos_r11': a11}
    return result


def _sum_in_image_order(total, per_image):
    for x in per_image:
        total += x
    return total


def evaluate_rows(rows_list, labels_list, min_overlap=(0.7, 0.7, 0.7)):
    """ the host form on parsed inputs: per image the (D_b, 36) rows and the (A_b, 16) labels """
    min_overlap = _check_min_overlap(min_overlap)
    overlaps = [image_overlaps(r, g) for r, g in zip(rows_list, labels_list)]
    A = max([np.asarray(g).reshape(-1, LABEL_COLS).shape[0] for g in labels_list] + [1])
    tp_scores = np.full((len(rows_list), 3, 3, A), np.nan, np.float32)
    n_gt = np.zeros((3, 3), np.int64)
    for b, (r, g, o) in enumerate(zip(rows_list, labels_list, overlaps)):
        s, n = match_image(r, g, o, min_overlap)
        tp_scores[b, :, :, :s.shape[2]] = s
        n_gt += n
    thr, n_thr = thresholds_of(tp_scores, n_gt)
    stats = np.zeros((3, 3, N_SAMPLE_PTS, 3), np.int64)
    sim = np.zeros((3, 3, N_SAMPLE_PTS), np.float64)
    for r, g, o in zip(rows_list, labels_list, overlaps):
        s, c = match_image(r, g, o, min_overlap, thr, n_thr)
        stats += s
        sim += c
    return summarise(stats, sim, thr, n_thr)


def _check_min_overlap(min_overlap):
    mo = np.asarray(min_overlap, np.float64).reshape(-1)
    if mo.shape != (3,) or not (mo >= 0.0).all():
        raise ValueError('min_overlap is three non-negative numbers (image, BEV, 3-D), got {!r}'.format(min_overlap))
    return mo


# ---------------------------------------------------------------------------------------------------- the device form
class DeviceChunk(object):
    """ some images of a dataset on the device: rows (B, D, 36) float32, labels (B, A, 16) float64, label_counts (B,) int32 and their
    overlaps (B, 4, D, A) float64 (launched, not waited for) """

    def __init__(self, rows, labels, label_counts, overlaps):
        self.rows, self.labels, self.label_counts, self.overlaps = rows, labels, label_counts, overlaps


def pack_labels(labels_list, A=None):
    """ per-image (n, 16) label arrays -> (B, A, 16) float64 zero-padded and the counts (B,) int32 """
    arrays = [np.asarray(g, np.float64).reshape(-1, LABEL_COLS) for g in labels_list]
    A = max([g.shape[0] for g in arrays] + [0]) if A is None else int(A)
    packed = np.zeros((len(arrays), A, LABEL_COLS), np.float64)
    for b, g in enumerate(arrays):
        packed[b, :g.shape[0]] = g
    return packed, np.array([g.shape[0] for g in arrays], np.int32)


def upload_chunk(rows, labels_list, device=None):
    """ rows (B, D, 36) -- a NumPy array, or a float32 tensor already on the device -- and the per-image labels: one upload, then the
    overlap launch on the current stream """
    import torch
    from ..backend import hip
    dev = hip.require_device() if device is None else device
    packed, counts = pack_labels(labels_list)
    rows_d = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float32)).to(dev, non_blocking=True)
    if rows_d.dim() != 3 or int(rows_d.shape[0]) != len(labels_list):
        raise ValueError('rows must be (B, D, {}) with one label array per image, got {} and {} label arrays'.format(
            POSE_COLS, tuple(rows_d.shape), len(labels_list)))
    labels_d = torch.as_tensor(packed).to(rows_d.device, non_blocking=True)
    counts_d = torch.as_tensor(counts).to(rows_d.device, non_blocking=True)
    return DeviceChunk(rows_d, labels_d, counts_d, hip.kitti_overlaps(rows_d, labels_d, counts_d))


def evaluate_chunks(chunks, min_overlap=(0.7, 0.7, 0.7)):
    """ the dataset level over DeviceChunks in image order (evaluate_kitti(device=True), RetinaNet3D.score_poses_on_frames): pass 1 on
    every chunk, the thresholds on the host, pass 2 on every chunk; the per-image results are summed on the host in image order """
    import torch
    from ..backend import hip
    min_overlap = _check_min_overlap(min_overlap)
    first = [hip.kitti_stats(c.rows, c.labels, c.label_counts, c.overlaps, min_overlap) for c in chunks]
    n_gt = np.zeros((3, 3), np.int64)
    scores = []
    for s, n in first:
        scores.append(s.cpu().numpy().reshape(s.shape[0], 3, 3, -1))
        n_gt += n.cpu().numpy().astype(np.int64).sum(axis=0)
    A = max([s.shape[3] for s in scores] + [1])
    tp_scores = np.full((sum(s.shape[0] for s in scores), 3, 3, A), np.nan, np.float32)
    at = 0
    for s in scores:
        tp_scores[at:at + s.shape[0], :, :, :s.shape[3]] = s
        at += s.shape[0]
    thr, n_thr = thresholds_of(tp_scores, n_gt)
    stats = np.zeros((3, 3, N_SAMPLE_PTS, 3), np.int64)
    sim = np.zeros((3, 3, N_SAMPLE_PTS), np.float64)
    if chunks:
        dev = chunks[0].rows.device
        thr_d, n_thr_d = torch.as_tensor(thr).to(dev), torch.as_tensor(n_thr).to(dev)
        second = [hip.kitti_stats(c.rows, c.labels, c.label_counts, c.overlaps, min_overlap, thr_d, n_thr_d) for c in chunks]
        for s, c in second:
            stats += s.cpu().numpy().astype(np.int64).sum(axis=0)
            _sum_in_image_order(sim, c.cpu().numpy())
    return summarise(stats, sim, thr, n_thr)


def chunk_images(D, A):
    """ the images per chunk whose overlaps (4 D A float64 each) stay below OVERLAP_WORKSPACE_BYTES """
    return max(1, min(32768, OVERLAP_WORKSPACE_BYTES // max(1, 4 * D * A * 8)))


def evaluate_rows_device(rows_list, labels_list, min_overlap=(0.7, 0.7, 0.7)):
    """ the device form on parsed inputs.  The chunks stay resident from the overlap launch to the end of pass 2. """
    import torch
    if not torch.cuda.is_available():
        raise ValueError('evaluate_kitti(device=True) runs csrc/kitti_eval.hip on a HIP device and none is visible: use device=False')
    min_overlap = _check_min_overlap(min_overlap)
    D = max([np.asarray(r).reshape(-1, POSE_COLS).shape[0] for r in rows_list] + [1])
    A = max([np.asarray(g).reshape(-1, LABEL_COLS).shape[0] for g in labels_list] + [0])
    if D > MAX_DETECTIONS or A > MAX_LABELS:
        raise ValueError('the device form takes up to {} detections and {} labels per image, got {} and {}: use device=False'.format(
            MAX_DETECTIONS, MAX_LABELS, D, A))
    step = chunk_images(D, A)
    chunks = []
    for at in range(0, len(rows_list), step):
        part = rows_list[at:at + step]
        rows = np.full((len(part), D, POSE_COLS), -1.0, np.float32)
        for b, r in enumerate(part):
            r = np.asarray(r, np.float32).reshape(-1, POSE_COLS)
            rows[b, :r.shape[0]] = r
        chunks.append(upload_chunk(rows, labels_list[at:at + step]))
    return evaluate_chunks(chunks, min_overlap)


# ---------------------------------------------------------------------------------------------------- the public entry
def evaluate_kitti(label_dir, result_dir=None, *, rows=None, device=False, min_overlap=(0.7, 0.7, 0.7)):
    """ KITTI's object benchmark for the class Car over the label files of `label_dir` (ORIGINAL label_2 files, sorted by name).
    The detections come from `result_dir` (the result file of the same name; a missing file is an image without detections) or from
    `rows`: per image the (D, 36) pose rows of predict_poses_on_batch (padding rows are -1), as a sequence in the order of the sorted
    label files or as a dict keyed by the file's stem.
    Returns {(metric, difficulty): {'ap_r40', 'ap_r11', 'thresholds', 'tp', 'fp', 'fn'}, ('aos', difficulty): {'aos_r40', 'aos_r11'}}
    with metric in 'image' 'bev' '3d' and difficulty in 'easy' 'moderate' 'hard'; tp, fp, fn are per threshold.
    device=False: NumPy.  device=True: csrc/kitti_eval.hip (up to 128 detections and 128 labels per image). """
    if (result_dir is None) == (rows is None):
        raise ValueError('give either result_dir or rows')
    names = sorted(f for f in os.listdir(label_dir) if f.endswith('.txt'))
    labels_list = [read_label_file(os.path.join(label_dir, f)) for f in names]
    if rows is None:
        rows_list = []
        for f in names:
            path = os.path.join(result_dir, f)
            rows_list.append(rows_from_results(read_result_file(path)) if os.path.isfile(path) else np.zeros((0, POSE_COLS), np.float32))
    else:
        rows_list = [rows[os.path.splitext(f)[0]] for f in names] if isinstance(rows, dict) else list(rows)
        if len(rows_list) != len(names):
            raise ValueError('{} row arrays for {} label files'.format(len(rows_list), len(names)))
    if device:
        return evaluate_rows_device(rows_list, labels_list, min_overlap)
    return evaluate_rows(rows_list, labels_list, min_overlap)


def summary_table(result):
    """ the devkit's summary: one line per metric with Easy / Moderate / Hard, AP|R40 (and AP|R11 in brackets) """
    lines = []
    for key, name in (('image', 'Car bbox AP'), ('bev', 'Car bev  AP'), ('3d', 'Car 3d   AP')):
        lines.append('{}: '.format(name) + '  '.join('{:7.4f} ({:7.4f})'.format(result[(key, d)]['ap_r40'], result[(key, d)]['ap_r11']) for d in DIFFICULTIES))
    lines.append('Car aos    : ' + '  '.join('{:7.4f} ({:7.4f})'.format(result[('aos', d)]['aos_r40'], result[('aos', d)]['aos_r11']) for d in DIFFICULTIES))
    return 'AP|R40 (AP|R11)   easy, moderate, hard\n' + '\n'.join(lines)


def result_as_json(result):
    """ the result dict with string keys and lists, for json.dump """
    return {'{}_{}'.format(*k): {n: (v.tolist() if isinstance(v, np.ndarray) else v) for n, v in e.items()} for k, e in result.items()}
