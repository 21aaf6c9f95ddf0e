"""
Suppression of duplicate cuboids: a greedy non-maximum suppression of the pose rows of one image by the overlap of the cuboids
themselves, in the bird's-eye view ('bev') or in 3-D ('3d') -- DESIGN.md section 4.26 is the specification, include/gpp.h
(gpp_cuboid_nms_f64) the contract.  The decode's NMS judges image rectangles; this one knows that two cars cannot stand on the same
piece of road.  There is no default threshold: nobody can measure one without trained weights, so the caller states it.

Two forms of one computation:
    suppress_rows_np        NumPy, no GPU and no library: the overlaps of all pairs at once (the clipping of utils/kitti_eval.py), the
                            greedy pass serial over the ranks, as the rule demands.
    suppress_rows_device    csrc/cuboid_nms.hip: one launch, one workgroup per image.

A row is a row of gpp_pose_f32: live iff its column 14 is >= 0; ranked by (score descending, row index ascending); kept iff no already
kept row overlaps it by more than the threshold (strict).  A suppressed row becomes -1 throughout, the padding every reader skips.
"""
import numpy as np

from . import kitti_eval

METRICS = ('bev', '3d')                     # include/gpp.h: GPP_CUBOID_NMS_BEV 0, GPP_CUBOID_NMS_3D 1
POSE_COLS = kitti_eval.POSE_COLS
MAX_DETECTIONS = kitti_eval.MAX_DETECTIONS  # what the device form takes per image


def metric_code(metric):
    if metric not in METRICS:
        raise ValueError("cuboid_nms: the metric must be 'bev' or '3d', got {!r}".format(metric))
    return METRICS.index(metric)


def check_option(option):
    """ the `cuboid_nms` option of load_model / RetinaNet3D: None, or (metric, threshold) -> None or (metric, float(threshold)) """
    if option is None:
        return None
    try:
        metric, threshold = option
    except (TypeError, ValueError):
        raise ValueError("cuboid_nms must be None or a pair (metric, threshold) such as ('bev', 0.3), got {!r}".format(option))
    metric_code(metric)
    return metric, check_threshold(threshold)


def check_threshold(threshold):
    threshold = float(threshold)
    if not 0.0 < threshold < 1.0:
        raise ValueError('cuboid_nms: the threshold must lie inside (0, 1), got {!r}'.format(threshold))
    return threshold


def pair_overlaps_np(rows, metric):
    """ rows (D, 36) float32 -> (D, D) float64: the overlap of every pair of live rows, symmetric -- for i < j row i takes the place of
    utils.kitti_eval.image_overlaps' detection and row j that of its label (row i's rectangle is clipped against row j's edges).  NaN
    where an operand is NaN; 0 on the diagonal and wherever a row is not live. """
    code = metric_code(metric)
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    D = rows.shape[0]
    out = np.zeros((D, D), np.float64)
    r = rows.astype(np.float64)
    live = np.flatnonzero(rows[:, 14] >= 0.0)
    a, c = np.triu_indices(live.size, 1)
    if a.size == 0:
        return out
    d, g = r[live[a]], r[live[c]]                                        # d: the lower row index
    dh, dw, dl, dtx, dty, dtz, dry = d[:, 30], d[:, 17], d[:, 18], d[:, 19], d[:, 31], d[:, 21], d[:, 32]
    gh, gw, gl, gtx, gty, gtz, gry = g[:, 30], g[:, 17], g[:, 18], g[:, 19], g[:, 31], g[:, 21], g[:, 32]
    with np.errstate(invalid='ignore', divide='ignore'):
        bad = np.isnan(np.stack([dw, dl, dtx, dtz, dry, gw, gl, gtx, gtz, gry])).any(axis=0)
        ok = np.flatnonzero(~bad)
        inter = np.zeros(a.size)
        if ok.size:
            inter[ok] = kitti_eval.rect_intersections(dl[ok], dw[ok], dtx[ok], dtz[ok], dry[ok], gl[ok], gw[ok], gtx[ok], gtz[ok], gry[ok])
        area_d, area_g = dl * dw, gl * gw
        if code == 0:
            o = inter / (area_d + area_g - inter)
        else:
            bad = bad | np.isnan(np.stack([dh, dty, gh, gty])).any(axis=0)
            iv = inter * kitti_eval.height_overlaps(dty, dh, gty, gh)
            o = iv / (area_d * dh + area_g * gh - iv)
        o[bad] = np.nan
    out[live[a], live[c]] = o
    out[live[c], live[a]] = o
    return out


def rank_order(rows):
    """ the live rows of one image in rank order: score descending, row index ascending (a NaN score ranks as -infinity) """
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    live = np.flatnonzero(rows[:, 14] >= 0.0)
    score = np.where(np.isnan(rows[live, 12]), -np.inf, rows[live, 12])
    return live[np.argsort(-score, kind='stable')]


def suppress_rows_np(rows, metric, threshold):
    """ rows (D, 36) float32 of one image -> (rows_out (D, 36) float32, count, suppressor (D,) int32): include/gpp.h,
    gpp_cuboid_nms_f64 """
    threshold = check_threshold(threshold)
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    over = pair_overlaps_np(rows, metric) > threshold                    # (a NaN overlap is above nothing)
    out = rows.copy()
    suppressor = np.full(rows.shape[0], -1, np.int32)
    kept = []                                                            # in rank order
    for d in rank_order(rows):
        by = [k for k in kept if over[d, k]]
        if by:
            suppressor[d] = by[0]
            out[d] = -1.0
        else:
            kept.append(int(d))
    return out, len(kept), suppressor


def suppress_batch_np(rows, metric, threshold):
    """ suppress_rows_np for (B, D, 36): -> (rows_out (B, D, 36), counts (B,) int32, suppressor (B, D) int32) """
    rows = np.asarray(rows, np.float32)
    rows = rows.reshape(-1, rows.shape[-2], POSE_COLS)
    res = [suppress_rows_np(r, metric, threshold) for r in rows]
    return (np.stack([x[0] for x in res]).reshape(rows.shape), np.array([x[1] for x in res], np.int32),
            np.stack([x[2] for x in res]).reshape(rows.shape[:2]).astype(np.int32))


def live_first(rows_b):
    """ one image's rows with the live ones (column 14 >= 0) in front, order kept: what the host writers, which take the first `count`
    rows of an image, read after a suppression (a suppressed row is padding in the middle of the table) """
    rows_b = np.asarray(rows_b, np.float32).reshape(-1, POSE_COLS)
    live = rows_b[:, 14] >= 0.0
    return np.concatenate([rows_b[live], rows_b[~live]], axis=0)


def suppress_detections(det, metric, threshold):
    """ the host path of bin/run_network.py: det = the dict of gpp_utils.recover_pose for one image -> (the dict without the suppressed
    detections, suppressor (n,) int32).  The rows are built from the dict with the KITTI fields of gpp_utils.kitti_lines. """
    from . import gpp_utils
    n = len(det['scores'])
    rows = np.zeros((n, POSE_COLS), np.float32)
    if n:
        X = gpp_utils.cuboid_corners(det)
        rows[:, 12] = det['scores']
        rows[:, 16:19] = det['dimensions']
        rows[:, 19:22] = det['locations']
        rows[:, 31] = X[:, 1, :].max(axis=1)
        rows[:, 30] = X[:, 1, :].max(axis=1) - X[:, 1, :].min(axis=1)
        rows[:, 32] = gpp_utils._wrap(np.asarray(det['angles'])[:, 1].astype(np.float64))
    _, _, suppressor = suppress_rows_np(rows, metric, threshold)
    keep = suppressor < 0
    out = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in det.items()}
    return out, suppressor


def suppress_rows_device(rows, metric, threshold):
    """ rows (B, D, 36): a NumPy array -> NumPy results, or a float32 device tensor -> device tensors (no synchronisation; the input is
    left alone).  Returns (rows_out (B, D, 36) float32, counts (B,) int32, suppressor (B, D) int32).  D <= 128. """
    import torch
    from ..backend import hip
    code, threshold = metric_code(metric), check_threshold(threshold)
    if isinstance(rows, torch.Tensor):
        if rows.dim() != 3 or not rows.is_contiguous():
            raise ValueError('suppress_rows_device: rows must be a dense (B, D, {}) tensor, got {}'.format(POSE_COLS, tuple(rows.shape)))
        return hip.cuboid_nms(rows, code, threshold)
    host = np.ascontiguousarray(rows, np.float32)
    if host.ndim != 3 or host.shape[2] != POSE_COLS:
        raise ValueError('suppress_rows_device: rows must be (B, D, {}), got {}'.format(POSE_COLS, host.shape))
    out, counts, suppressor = hip.cuboid_nms(torch.as_tensor(host).to(hip.require_device()), code, threshold)
    return out.cpu().numpy(), counts.cpu().numpy(), suppressor.cpu().numpy()
