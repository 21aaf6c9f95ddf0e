"""
Distil a plane database: from a pool of candidate planes (the 22k file, or per-frame road fits of one's own) and a labelled dataset, the K
planes that ground-plane polling on that dataset loses least with -- DESIGN.md section 4.21 is the specification.  The reference ships
five fixed databases and tells the user to "replace road_planes_database.mat with relevant files of your own"; this module makes one.

    cost_table     labels -> keypoints (gpp_label_prep_f64) -> the (object, plane) table of 16-bit keys (gpp_poll_costs_u16, csrc/plane_db.hip)
    select         greedy facility location on the table on the device (gpp_plane_select)
    select_np      the same in NumPy integers: equal to the kernel entry for entry
    distil         label_2 + calib directories and a pool -> the chosen rows of the pool in pick order, with the objective's trace
    write_database the rows as a .mat that the rest of the project (and the reference) reads

The key of a pair: 65535 if the plane puts the object behind the camera or its residual is not finite, else
(6 - votes) * 8192 + min(floor(1024 * residual sum in metres), 8191) -- the order in which polling itself ranks planes.  The objective is
the sum over the objects of the best key among the chosen planes; every pick takes the plane that lowers it most (the first such plane),
so the picks of a run are a prefix of the picks of every longer run.

With objective='location' (opt-in) the selection minimises what an object finally loses: the location error of
the plane that polling itself would pick among the chosen planes.  A second table holds the location error of every pair in 1/256 m
(gpp_pose_costs_u16; pair_costs_np is its NumPy form), and the rule follows polling: a row is served by the chosen plane of the smallest
key, the earlier pick on equal keys, and pays that plane's error (gpp_plane_select_polled; select_polled_np, polled_state_np).  Gains
are signed there: the objective is not monotone, the rule is a greedy heuristic, and only its first pick is provably the best one.

The device entry points raise GppError without a GPU, like polling_ceiling; select_np, select_polled_np and pair_costs_np need nothing
but NumPy.
"""
import os

import numpy as np

from . import kitti_eval
from .label_prep import CAR, _check_alpha, _load_planes, _upload, read_calibration

INVALID = 65535                                             # GPP_PLANE_COST_INVALID (include/gpp.h)
VOTE_STEP = 8192                                            # key = (6 - votes) * VOTE_STEP + residual quantum
QUANTA_PER_M = 1024.0
DATABASE_KEY = 'road_planes_database'
ERR_PER_M = 256.0                                           # errs: the location error in quanta of 1/256 m ...
ERR_MAX = 65534                                             # ... saturating here; 65535 where the key is
OBJECTIVES = ('poll', 'location')


# ---------------------------------------------------------------------------------------------------- the host form of the selection
def select_np(table, k):
    """ greedy facility location on table (O, M) of uint16 keys, k picks, in NumPy integers: the host form of gpp_plane_select.
    Returns {'chosen' (k,) int32, 'trace' (k + 1,) uint64, 'best' (O,) uint16, 'count' int}: pick j takes the FIRST plane of the largest
    gain sum_o max(0, best[o] - table[o][p]); a largest gain of 0 ends the run (chosen -1 from there on, the trace repeats). """
    table = np.asarray(table)
    if table.ndim != 2 or table.dtype != np.uint16:
        raise ValueError('table must be (O, M) uint16, got {} {}'.format(table.shape, table.dtype))
    O, M = table.shape
    k = int(k)
    if O < 1 or M < 1 or k < 1 or k > M:
        raise ValueError('O = {}, M = {}, k = {}: needs O >= 1 and 1 <= k <= M'.format(O, M, k))
    t = table.astype(np.int32)
    best = np.full(O, INVALID, np.int32)
    chosen = np.full(k, -1, np.int32)
    trace = np.empty(k + 1, np.uint64)
    trace[0] = INVALID * O
    count = 0
    for j in range(k):
        gain = np.maximum(best[:, None] - t, 0).sum(axis=0, dtype=np.int64)
        p = int(np.argmax(gain))                             # the first maximum
        if gain[p] == 0:
            break
        chosen[j], count = p, j + 1
        best = np.minimum(best, t[:, p])
        trace[j + 1] = int(trace[j]) - int(gain[p])
    trace[count + 1:] = trace[count]
    return {'chosen': chosen, 'trace': trace, 'best': best.astype(np.uint16), 'count': count}


def objective(table, chosen):
    """ sum over the rows of the smallest key among the columns `chosen` (65535 per row when there are none): what trace[len(chosen)] holds """
    table = np.asarray(table)
    chosen = [int(p) for p in chosen if int(p) >= 0]
    if not chosen:
        return INVALID * table.shape[0]
    return int(table[:, chosen].min(axis=1).astype(np.int64).sum())


def best_summary(best):
    """ what `best` (O,) uint16 says about the chosen planes: the share of objects whose best plane has all six votes, and the median over
    the objects some plane serves of that plane's residual in metres per segment (the quantised residual sum / 6, as gpp_poll_f32
    reports residuals; the quantum saturates at 8191 / 1024 m) """
    best = np.asarray(best).astype(np.int64)
    served = best[best < INVALID]
    return {'objects': int(best.size), 'served': int(served.size),
            'six_vote_share': float((best < VOTE_STEP).sum()) / best.size if best.size else 0.0,
            'median_residual_m': float(np.median((served % VOTE_STEP) / QUANTA_PER_M / 6.0)) if served.size else float('nan')}


# ---------------------------------------------------------------------------------------------------- the polled location objective
def _check_pair(keys, errs):
    keys, errs = np.asarray(keys), np.asarray(errs)
    if keys.ndim != 2 or keys.dtype != np.uint16 or errs.dtype != np.uint16 or errs.shape != keys.shape:
        raise ValueError('keys and errs must be (O, M) uint16 of one shape, got {} {} and {} {}'.format(keys.shape, keys.dtype, errs.shape, errs.dtype))
    return keys, errs


def select_polled_np(keys, errs, k):
    """ the host form of gpp_plane_select_polled on keys, errs (O, M) uint16, k picks, in NumPy integers.  Returns {'chosen' (k,) int32,
    'trace' (k + 1,) uint64, 'best' (O,) uint16, 'cur' (O,) uint16, 'count' int}: best[o] is the smallest key among the picks so far,
    cur[o] the error of the plane that holds it; pick j takes the FIRST plane of the largest signed gain
    sum over o with keys[o][p] < best[o] of (cur[o] - errs[o][p]); a largest gain of at most 0 ends the run. """
    keys, errs = _check_pair(keys, errs)
    O, M = keys.shape
    k = int(k)
    if O < 1 or M < 1 or k < 1 or k > M:
        raise ValueError('O = {}, M = {}, k = {}: needs O >= 1 and 1 <= k <= M'.format(O, M, k))
    kt, et = keys.astype(np.int32), errs.astype(np.int32)
    best = np.full(O, INVALID, np.int32)
    cur = np.full(O, INVALID, np.int32)
    chosen = np.full(k, -1, np.int32)
    trace = np.empty(k + 1, np.uint64)
    trace[0] = INVALID * O
    count = 0
    for j in range(k):
        gain = np.where(kt < best[:, None], cur[:, None] - et, 0).sum(axis=0, dtype=np.int64)
        p = int(np.argmax(gain))                             # the first maximum
        if gain[p] <= 0:
            break
        chosen[j], count = p, j + 1
        takes = kt[:, p] < best
        best = np.where(takes, kt[:, p], best)
        cur = np.where(takes, et[:, p], cur)
        trace[j + 1] = int(trace[j]) - int(gain[p])
    trace[count + 1:] = trace[count]
    return {'chosen': chosen, 'trace': trace, 'best': best.astype(np.uint16), 'cur': cur.astype(np.uint16), 'count': count}


def polled_state_np(keys, errs, order):
    """ the replay: (best, cur) (O,) uint16 after the planes `order` (column indices; negative ones are skipped) in that order -- per row
    the smallest key and the error of the FIRST plane of the order that holds it, as polling on the written file picks.  cur.sum() is
    what trace[len(order)] holds; it scores any database under this measure, a shipped one included. """
    keys, errs = _check_pair(keys, errs)
    best = np.full(keys.shape[0], INVALID, np.uint16)
    cur = np.full(keys.shape[0], INVALID, np.uint16)
    for p in order:
        p = int(p)
        if p < 0:
            continue
        takes = keys[:, p] < best
        best = np.where(takes, keys[:, p], best)
        cur = np.where(takes, errs[:, p], cur)
    return best, cur


def location_summary(cur):
    """ what `cur` (O,) uint16 says: the objects some plane serves, and over those the mean and the median location error in metres
    (quanta of 1/256 m, saturating just below 256 m) """
    cur = np.asarray(cur).astype(np.int64)
    served = cur[cur < INVALID]
    return {'objects': int(cur.size), 'served': int(served.size),
            'mean_location_m': float(served.mean() / ERR_PER_M) if served.size else float('nan'),
            'median_location_m': float(np.median(served / ERR_PER_M)) if served.size else float('nan')}


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _norm3(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _sub3(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _scale3(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def pair_costs_np(boxes, dims, orient, P_inv, want, planes, thr=0.7, return_locations=False):
    """ the NumPy form of gpp_pose_costs_u16 for every row of a batch: boxes (B, D, 12), dims (B, D, 3), orient (B, D), P_inv (B, 4, 3),
    want (B, D, 3), planes (M, 4) -> (keys, errs), both (B * D, M) uint16.  float32, component by component, every operation separate, in
    the order of csrc/poll_eval.h and csrc/pose_eval.h (no np.linalg.norm, no np.cross: their sums associate differently).
    With return_locations also the unquantised locations (B * D, M, 3) and the keypoints X_l, X_m, X_r, X_t (B * D, M, 4, 3), float32. """
    F = np.float32
    boxes, dims, P_inv, want = (np.asarray(a, F) for a in (boxes, dims, P_inv, want))
    orient = np.asarray(orient)
    planes = np.asarray(planes, F).reshape(-1, 4)
    B, D = orient.shape
    thr = F(thr)
    with np.errstate(all='ignore'):
        # canonical planes: normal up, unit norm
        direction = -np.sign(planes[:, 1])
        a, b, c, d = (planes[:, k] * direction for k in range(4))
        nn = np.sqrt((a * a + b * b) + c * c)
        n = (a / nn, b / nn, c / nn)                                                   # (M,) each
        nd = -(d / nn)
        # rays of the four keypoints, (B, D, 1) each component
        Pi = P_inv[:, None, :, :]
        ray = []
        for k in range(4):
            x, y = boxes[..., 4 + 2 * k], boxes[..., 5 + 2 * k]
            r = [(Pi[..., i, 0] * x + Pi[..., i, 1] * y) + Pi[..., i, 2] * F(1.0) for i in range(3)]
            sg = np.sign(r[2])
            ray.append(tuple((r[i] * sg)[..., None] for i in range(3)))
        X = [_scale3(ray[k], np.abs(nd / _dot3(n, ray[k]))) for k in range(3)]          # (B, D, M) each component
        zc = _cross3(_sub3(X[0], X[1]), _sub3(X[2], X[1]))[1]
        perp = _cross3(ray[3], _cross3(n, ray[3]))
        X.append(_sub3(X[1], _scale3(n, _dot3(perp, X[1]) / _dot3(perp, n))))
        # poll targets
        h, w, l = dims[..., 0], dims[..., 1], dims[..., 2]
        hw, wl, hl = np.sqrt(h * h + w * w), np.sqrt(w * w + l * l), np.sqrt(h * h + l * l)
        oh = [(orient == k).astype(F) for k in range(4)]
        mix = lambda p, q, r, t: ((oh[0] * p + oh[1] * q) + oh[2] * r) + oh[3] * t      # noqa: E731
        targets = [h, mix(l, w, w, l), mix(w, l, l, w), wl, mix(hl, hw, hw, hl), mix(hw, hl, hl, hw)]
        votes = res = None
        for (i, j), t in zip(((1, 3), (0, 1), (1, 2), (0, 2), (0, 3), (2, 3)), targets):
            r = np.abs(_norm3(_sub3(X[i], X[j])) - t[..., None])
            v = np.where(r > thr, F(0.0), F(1.0)).astype(F)
            votes = v if votes is None else votes + v
            res = r if res is None else res + r
        invalid = (zc < F(0.0)) | ~(res < np.finfo(F).max) | (orient < 0)[..., None]
        s = res * F(1024.0)
        q = np.where(s < F(8191.0), np.where(invalid, F(0.0), s).astype(np.int64), 8191)
        keys = np.where(invalid, INVALID, (6 - np.where(invalid, F(0.0), votes).astype(np.int64)) * VOTE_STEP + q)
        # the location of pose recovery's live branch (gpp_utils.recover_pose), by components
        o = orient[..., None]
        use_l = (o == 0) | (o == 3)
        X_m, X_t = X[1], X[3]
        X_s = tuple(np.where(use_l, X[0][i], X[2][i]) for i in range(3))
        hh = _norm3(_sub3(X_t, X_m))
        e = _norm3(_sub3(X_s, X_m))
        y_dir = tuple(v / hh for v in _sub3(X_m, X_t))
        sx = np.where((o == 0) | (o == 1), F(1.0), F(-1.0)).astype(F)
        x_dir = tuple(v / e for v in _scale3(_sub3(X_m, X_s), sx))
        z_dir = _cross3(x_dir, y_dir)
        sz = np.where((o == 0) | (o == 2), F(1.0), F(-1.0)).astype(F)
        wide = w[..., None]
        loc = tuple((X_m[i] + X_s[i]) / F(2.0) + ((sz * z_dir[i]) * wide) / F(2.0) for i in range(3))
        dist = _norm3(_sub3(loc, tuple(want[..., i][..., None] for i in range(3))))
        se = dist * F(ERR_PER_M)
        under = se < F(ERR_MAX)
        qe = np.where(under, np.where(under, se, F(0.0)).astype(np.int64), ERR_MAX)
        errs = np.where(invalid, INVALID, qe)
    M = planes.shape[0]
    keys, errs = keys.reshape(B * D, M).astype(np.uint16), errs.reshape(B * D, M).astype(np.uint16)
    if return_locations:
        assert all(v.dtype == F for v in loc)
        points = np.stack([np.stack(np.broadcast_arrays(*X[k]), axis=-1) for k in range(4)], axis=-2)
        return keys, errs, np.stack(loc, axis=-1).reshape(B * D, M, 3), points.reshape(B * D, M, 4, 3)
    return keys, errs


# ---------------------------------------------------------------------------------------------------- the device side
def cost_table(labels_list, P_list, pool, det_types=CAR, thr=0.7, chunk_images=None, errors=False):
    """ the cost table of a dataset on the device: per image the (n, 16) labels and the (3, 4) matrix, pool (M, 4) -> (table, M) with
    table an (O, pitch) int16 device tensor of uint16 keys, one row per label that is a detection of `det_types` (in image, then label
    order), pitch = M rounded up to 8, the pad columns 65535.  Chunked as polling_ceiling is: per chunk labels, trig, P and pinv(P) go up
    once, gpp_label_prep_f64 (own_box) fills the decode layout, the rows with orient >= 0 are listed on the device and
    gpp_poll_costs_u16 fills its rows.  Raises GppError without a GPU, MemoryError when the table does not fit the free device memory.
    With `errors` -> (keys, errs, M): gpp_pose_costs_u16 fills both tables of section 4.23 (keys the table above, errs the location
    errors against the labels' columns 11:14), and the memory check counts both. """
    import torch
    from ..backend import hip
    dev = hip.require_device()
    if len(labels_list) != len(P_list):
        raise ValueError('{} label arrays and {} matrices'.format(len(labels_list), len(P_list)))
    pool32 = _load_planes(pool)
    M = pool32.shape[0]
    planes_d = torch.as_tensor(pool32).to(dev)
    A = max([np.asarray(g).reshape(-1, kitti_eval.LABEL_COLS).shape[0] for g in labels_list] + [1])
    if A > kitti_eval.MAX_LABELS:
        raise ValueError('the device form takes up to {} labels per image, got {}'.format(kitti_eval.MAX_LABELS, A))
    step = kitti_eval.chunk_images(A, A) if chunk_images is None else max(1, int(chunk_images))
    parts = []
    for at in range(0, len(labels_list), step):
        part_labels, part_P = labels_list[at:at + step], P_list[at:at + step]
        labels_d, counts_d, P_d, trig_d = _upload(part_labels, part_P, A, dev)
        pinv = np.stack([np.linalg.pinv(np.asarray(P, np.float64).reshape(3, 4)) for P in part_P]).astype(np.float32)
        pinv_d = torch.as_tensor(pinv).to(dev, non_blocking=True)
        _, (boxes, dims, _, _, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, det_types, True, True)
        rows = torch.nonzero(orient.reshape(-1) >= 0).reshape(-1).to(torch.int32)          # ascending: image, then label order
        want_d = None
        if errors:                                                                         # the labels' locations, float32 once, on the host
            want = kitti_eval.pack_labels(part_labels, A)[0][..., 11:14].astype(np.float32)
            want_d = torch.as_tensor(np.ascontiguousarray(want)).to(dev, non_blocking=True)
        parts.append((boxes, dims, orient, pinv_d, rows, want_d))
    O = sum(int(p[4].numel()) for p in parts)
    pitch = hip.table_pitch(M)
    free = torch.cuda.mem_get_info(dev)[0]
    tables = 2 if errors else 1
    if O * pitch * 2 * tables > free:
        raise MemoryError('the cost table{} of {} objects x {} planes need{} {:.2f} GB, {:.2f} GB of device memory are free: '
                          'use a smaller pool or fewer labels'.format('s' if errors else '', O, M, '' if errors else 's',
                                                                      O * pitch * 2 * tables / 1e9, free / 1e9))
    table = torch.full((O, pitch), -1, dtype=torch.int16, device=dev)                      # int16 -1 = the key 65535
    errs = torch.full((O, pitch), -1, dtype=torch.int16, device=dev) if errors else None
    at = 0
    for boxes, dims, orient, pinv_d, rows, want_d in parts:
        if rows.numel():
            if errors:
                at += hip.pose_costs(boxes, dims, orient, pinv_d, want_d, planes_d, table, errs, rows, at, thr)
            else:
                at += hip.poll_costs(boxes, dims, orient, pinv_d, planes_d, table, rows, at, thr)
    return (table, errs, M) if errors else (table, M)


def select(table, M, k):
    """ gpp_plane_select on a device table -> the dict of select_np (NumPy, fetched once at the end) """
    import torch
    from ..backend import hip
    chosen, trace, best, count = hip.plane_select(table, M, k)
    torch.cuda.synchronize(table.device)
    return {'chosen': chosen.cpu().numpy(), 'trace': trace.cpu().numpy().view(np.uint64), 'best': best.cpu().numpy().view(np.uint16),
            'count': int(count.item())}


def select_polled(keys, errs, M, k):
    """ gpp_plane_select_polled on device tables -> the dict of select_polled_np (NumPy, fetched once at the end) """
    import torch
    from ..backend import hip
    chosen, trace, best, cur, count = hip.plane_select_polled(keys, errs, M, k)
    torch.cuda.synchronize(keys.device)
    return {'chosen': chosen.cpu().numpy(), 'trace': trace.cpu().numpy().view(np.uint64), 'best': best.cpu().numpy().view(np.uint16),
            'cur': cur.cpu().numpy().view(np.uint16), 'count': int(count.item())}


def _result(pool, picked, objects):
    count = picked['count']
    indices = picked['chosen'][:count].copy()
    out = dict(best_summary(picked['best']), planes=np.ascontiguousarray(np.asarray(pool).reshape(-1, 4)[indices]), indices=indices,
               trace=picked['trace'], count=count, objects=objects, best=picked['best'])
    if 'cur' in picked:
        out.update(location_summary(picked['cur']), cur=picked['cur'], objective='location')
    return out


def _prefix_summary(short):
    return dict(best_summary(short['best']), **(location_summary(short['cur']) if 'cur' in short else {}))


def distil_rows(labels_list, P_list, pool, k, device=True, det_types=CAR, thr=0.7, chunk_images=None, report=False, objective='poll'):
    """ distil on arrays already in memory: per image the (n, 16) labels (kitti_eval.read_label_file) and the (3, 4) camera matrix, pool
    (M, 4) or the path of a .mat -> dict
        planes   (count, 4)  the chosen rows of the pool, verbatim, in pick order, in the pool's own dtype (not canonicalised)
        indices  (count,)    their rows in the pool;  count <= k: the run ends when no plane lowers the objective
        trace    (k + 1,)    uint64, the objective after 0 .. k picks: every prefix of `planes` is the distillation of its length
        objects, served, six_vote_share, median_residual_m, best: best_summary of the final state
        prefixes (with `report`): {n: best_summary} of the prefixes of 1, 10, 100 ... planes -- each a shorter run of the selection
    The cost table is always made on the device; device=False runs the selection in NumPy (select_np) instead of gpp_plane_select.
    objective='location' (section 4.23): both tables (gpp_pose_costs_u16) and gpp_plane_select_polled, or select_polled_np with
    device=False.  `trace` is then the sum of the polled location errors in 1/256 m, `best` still the smallest key per object, and the
    dict gains cur (O,) uint16, mean_location_m, median_location_m (location_summary) and objective; the prefixes carry them too. """
    if objective not in OBJECTIVES:
        raise ValueError("objective must be 'poll' or 'location', got {!r}".format(objective))
    if isinstance(pool, (str, bytes, os.PathLike)):
        import scipy.io
        pool = scipy.io.loadmat(pool)[DATABASE_KEY]
    pool = np.asarray(pool)
    if pool.ndim != 2 or pool.shape[1] != 4 or pool.shape[0] < 1:
        raise ValueError('the pool must be (M, 4) with M >= 1, got {}'.format(pool.shape))
    k = int(k)
    if k < 1 or k > pool.shape[0]:
        raise ValueError('{} planes asked of a pool of {}'.format(k, pool.shape[0]))
    errs = None
    if objective == 'location':
        table, errs, M = cost_table(labels_list, P_list, pool, det_types, thr, chunk_images, errors=True)
    else:
        table, M = cost_table(labels_list, P_list, pool, det_types, thr, chunk_images)
    O = int(table.shape[0])
    if O < 1:
        raise ValueError('the dataset has no object of the asked types in front of the camera')
    host = None if device else table[:, :M].cpu().numpy().view(np.uint16)
    if errs is not None:
        host_e = None if device else errs[:, :M].cpu().numpy().view(np.uint16)
        run = (lambda n: select_polled(table, errs, M, n)) if device else (lambda n: select_polled_np(host, host_e, n))
    else:
        run = (lambda n: select(table, M, n)) if device else (lambda n: select_np(host, n))
    picked = run(k)
    result = _result(pool, picked, O)
    if report:
        result['prefixes'] = {}
        for n in prefix_sizes(picked['count'])[:-1]:
            short = run(n)
            if not np.array_equal(short['chosen'], picked['chosen'][:n]):
                raise RuntimeError('the run of {} picks is no prefix of the run of {}'.format(n, k))
            result['prefixes'][n] = _prefix_summary(short)
    return result


def distil(label_dir, calib_dir, pool, k, device=True, det_types=CAR, thr=0.7, report=False, objective='poll'):
    """ distil_rows on the label_2 files of `label_dir` (sorted by name) and the calibration files of the same names in `calib_dir` """
    files = sorted(f for f in os.listdir(label_dir) if f.endswith('.txt'))
    labels_list = [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in files]
    P_list = [read_calibration(os.path.join(calib_dir, f)) for f in files]
    for f, g, P in zip(files, labels_list, P_list):
        try:
            _check_alpha(g, P)
        except ValueError as e:
            raise ValueError('{}: {}'.format(os.path.join(label_dir, f), e))
    return distil_rows(labels_list, P_list, pool, k, device, det_types, thr, report=report, objective=objective)


# ---------------------------------------------------------------------------------------------------- files
def write_database(path, planes):
    """ planes (N, 4) -> a .mat under the key road_planes_database, as the shipped databases are stored (utils.label_prep._load_planes,
    utils.synthetic.load_plane_database and the reference's run_network.py read it back) """
    import scipy.io
    planes = np.asarray(planes)
    if planes.ndim != 2 or planes.shape[1] != 4 or planes.shape[0] < 1:
        raise ValueError('planes must be (N, 4) with N >= 1, got {}'.format(planes.shape))
    scipy.io.savemat(path, {DATABASE_KEY: planes})


def prefix_sizes(count):
    """ 1, 10, 100 ... below `count`, then `count` itself """
    return sorted({10 ** e for e in range(0, 10) if 10 ** e < count} | ({count} if count > 0 else set()))


def prefix_report(result):
    """ one line per power of ten of the prefix and one for the whole run: planes, the objective and, where known (the whole run; the
    prefixes of a run made with `report`), the six-vote share and the median residual """
    lines = []
    if result.get('objective') == 'location':                # the objective in metres per object, the polled location error where known
        for n in prefix_sizes(result['count']):
            s = result if n == result['count'] else result.get('prefixes', {}).get(n)
            where = '   location error mean {:.3f} m   median {:.3f} m'.format(s['mean_location_m'], s['median_location_m']) if s else ''
            lines.append('{:8d} planes   objective {:16d}   per object {:10.4f} m{}'.format(
                n, int(result['trace'][n]), int(result['trace'][n]) / ERR_PER_M / max(1, result['objects']), where))
        return lines
    for n in prefix_sizes(result['count']):
        s = result if n == result['count'] else result.get('prefixes', {}).get(n)
        share = '   six votes {:7.2%}   median residual {:.4f} m'.format(s['six_vote_share'], s['median_residual_m']) if s else ''
        lines.append('{:8d} planes   objective {:16d}   per object {:10.2f}{}'.format(
            n, int(result['trace'][n]), int(result['trace'][n]) / max(1, result['objects']), share))
    return lines
