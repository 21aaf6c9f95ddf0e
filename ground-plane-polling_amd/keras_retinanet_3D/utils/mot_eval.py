"""
CLEAR-MOT scoring of tracks for the class Car (neighbouring class Van): per frame the OPTIMAL one-to-one assignment of the tracker's rows to
the labels, then identity switches, fragmentations, mostly tracked / mostly lost, MOTA and MOTP -- DESIGN.md section 4.29 is the
specification, a restatement of the KITTI tracking devkit's CLEAR-MOT.  Parity with the devkit itself is UNPINNED (it is not part of this
repository).  include/gpp.h (gpp_mot_assign, gpp_mot_clear) is the device form's contract.

Two forms of one computation:
    device=False    NumPy, no GPU and no library: the overlaps of utils/kitti_eval.image_overlaps, the assignment vectorised over the
                    columns and serial over the steps, as the rule demands.
    device=True     csrc/mot_eval.hip: gpp_kitti_overlaps_f64 per chunk of frames, then one launch for the assignments of all frames and
                    one for the trajectories of all sequences; only codes and integer counts come back.
Both end in the same host code (summarise), fed with the same integers.

A sequence's labels are (labels_per_frame, track_ids_per_frame): per frame an (n, 16) float64 array as utils/kitti_eval.read_label_file
gives it and the (n,) track_ids of its lines.  A sequence's tracks are (rows, ids): per frame the (D, 36) float32 pose rows and the (D,)
tracker ids -- as lists, as arrays (N, D, 36) and (N, D), or as the DEVICE tensors utils/track.track_rows_device returns (device form
only; they are scored where they lie).  A row is a track's row iff its column 14 is >= 0 and its id is >= 0.
"""
import os

import numpy as np

from . import kitti_eval

METRICS = kitti_eval.METRICS                # the plane of the overlaps: 'image' 0, 'bev' 1, '3d' 2
POSE_COLS, LABEL_COLS = kitti_eval.POSE_COLS, kitti_eval.LABEL_COLS
MAX_ROWS = kitti_eval.MAX_DETECTIONS        # rows and labels per frame, both forms: n * 2^20 < BIG needs n <= 128
MAX_LABELS = kitti_eval.MAX_LABELS
SCALE_BITS = 20                             # GPP_MOT_SCALE_BITS
SCALE = 1 << SCALE_BITS
BIG = 1 << 28                               # GPP_MOT_BIG
MAX_TRAJECTORIES = 1024                     # GPP_MOT_MAX_TRAJECTORIES: per sequence, device form
DEFAULTS = {'min_overlap': 0.5, 'max_occlusion': 2.0, 'max_truncation': 0.0, 'min_height': 25.0}       # the devkit's values
COUNTING, IGNORED, DONTCARE, OUT = 0, 1, 2, 3                                                           # a label's status
L_NONE, L_TP, L_FN, L_IGNORED_MATCHED, L_IGNORED_UNMATCHED = range(5)                                   # label_outcome
R_NONE, R_TP, R_IGNORED, R_FP, R_LOW, R_DONTCARE = range(6)                                             # row_outcome
FRAME_COUNTS = ('tp', 'fp', 'fn', 'n_gt', 'sum_k', 'cost', 'labels_in_play', 'rows')                    # frame_counts' columns
SEQ_COUNTS = ('tp', 'fp', 'fn', 'n_gt', 'sum_k', 'cost', 'ids', 'frag', 'mt', 'pt', 'ml', 'trajectories', 'frames')
_INF = np.iinfo(np.int64).max


def check_params(metric='image', min_overlap=0.5, max_occlusion=2.0, max_truncation=0.0, min_height=25.0):
    if metric not in METRICS:
        raise ValueError("the metric must be 'image', 'bev' or '3d', got {!r}".format(metric))
    values = {'min_overlap': float(min_overlap), 'max_occlusion': float(max_occlusion), 'max_truncation': float(max_truncation),
              'min_height': float(min_height)}
    if any(np.isnan(v) for v in values.values()) or not 0.0 <= values['min_overlap'] <= 1.0:
        raise ValueError('min_overlap must lie inside [0, 1] and no limit may be NaN, got {!r}'.format(values))
    return dict(values, metric=metric)


# ---------------------------------------------------------------------------------------------------- files
def read_tracking_labels(path):
    """ KITTI label_02 lines, `frame track_id type truncated occluded alpha x1 y1 x2 y2 h w l x y z r_y` -> (labels_per_frame,
    track_ids_per_frame) for the frames 0 .. the largest frame named: (n, 16) float64 arrays as utils/kitti_eval.read_label_file gives
    them (type code, truncation, occlusion, alpha, box, h w l, x y z, r_y, 0) and (n,) int64 track_ids, in line order """
    per_frame = {}
    with open(path, 'r') as f:
        for n, line in enumerate(f):
            fields = line.split()
            if not fields:
                continue
            if len(fields) not in (17, 18):
                raise ValueError('{}:{}: a tracking label line has 17 fields, got {}'.format(path, n + 1, len(fields)))
            frame, track_id = int(fields[0]), int(fields[1])
            if frame < 0:
                raise ValueError('{}:{}: frame {}'.format(path, n + 1, frame))
            row = np.zeros(LABEL_COLS, np.float64)
            row[0] = kitti_eval.TYPE_CODES.get(fields[2], 3)
            row[1:15] = [float(v) for v in fields[3:17]]
            per_frame.setdefault(frame, []).append((row, track_id))
    N = max(per_frame) + 1 if per_frame else 0
    labels = [np.array([r for r, _ in per_frame.get(k, [])], np.float64).reshape(-1, LABEL_COLS) for k in range(N)]
    ids = [np.array([t for _, t in per_frame.get(k, [])], np.int64) for k in range(N)]
    return labels, ids


def read_track_file(path):
    """ the lines utils/track.tracking_lines writes, `frame id Car -1 -1 alpha x1 y1 x2 y2 h w l x y z r_y score` -> (rows_per_frame,
    ids_per_frame) for the frames 0 .. the largest frame named: (n, 36) float32 pose rows (utils/kitti_eval.rows_from_results) and (n,)
    int32 ids, in line order.  Lines of another type than Car are dropped; a line without a score scores 1. """
    per_frame = {}
    with open(path, 'r') as f:
        for n, line in enumerate(f):
            fields = line.split()
            if not fields:
                continue
            if len(fields) not in (17, 18):
                raise ValueError('{}:{}: a track line has 17 or 18 fields, got {}'.format(path, n + 1, len(fields)))
            frame, track_id = int(fields[0]), int(fields[1])
            if frame < 0:
                raise ValueError('{}:{}: frame {}'.format(path, n + 1, frame))
            if fields[2] != 'Car':
                continue
            row = np.zeros(LABEL_COLS, np.float64)
            row[1:15] = [float(v) for v in fields[3:17]]
            row[15] = float(fields[17]) if len(fields) == 18 else 1.0
            per_frame.setdefault(frame, []).append((row, track_id))
    N = max(per_frame) + 1 if per_frame else 0
    rows = [kitti_eval.rows_from_results(np.array([r for r, _ in per_frame.get(k, [])], np.float64).reshape(-1, LABEL_COLS)) for k in range(N)]
    ids = [np.array([t for _, t in per_frame.get(k, [])], np.int32) for k in range(N)]
    return rows, ids


# ---------------------------------------------------------------------------------------------------- packing
class Packed(object):
    """ S sequences as the arrays both forms walk: labels (N, A, 16) float64, label_counts (N,) int32, traj (N, A) int32, rows (N, D, 36)
    float32 and ids (N, D) int32 (NumPy arrays, or device tensors), seq_start (S + 1,), and per sequence the track_ids of its trajectories """

    def __init__(self, labels, label_counts, traj, rows, ids, seq_start, traj_ids):
        self.labels, self.label_counts, self.traj, self.rows, self.ids = labels, label_counts, traj, rows, ids
        self.seq_start, self.traj_ids = seq_start, traj_ids


def _is_tensor(x):
    return hasattr(x, 'is_cuda')


def _frames_of(rows):
    return int(rows.shape[0]) if hasattr(rows, 'shape') else len(rows)


def pack_sequences(labels, tracks):
    """ labels: per sequence (labels_per_frame, track_ids_per_frame); tracks: per sequence (rows, ids) -> Packed.  A sequence has as many
    frames as the longer of the two.  ValueError: a (frame, track_id) that two Car or Van labels share, a tracker id twice in a frame (host
    arrays; device tensors come from the tracker, which gives an id once), more than 128 labels or rows in a frame. """
    if len(labels) != len(tracks):
        raise ValueError('{} sequences of labels, {} of tracks'.format(len(labels), len(tracks)))
    on_device = any(_is_tensor(t[0]) for t in tracks)
    if on_device and not all(_is_tensor(t[0]) and _is_tensor(t[1]) for t in tracks):
        raise ValueError('the tracks are device tensors in every sequence or in none')
    frames = [max(len(g[0]), _frames_of(t[0])) for g, t in zip(labels, tracks)]
    seq_start = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    N = int(seq_start[-1])
    # ---- labels
    label_list, traj_list, traj_ids = [], [], []
    for s, (per_frame, ids_per_frame) in enumerate(labels):
        if len(per_frame) != len(ids_per_frame):
            raise ValueError('sequence {}: {} frames of labels, {} of track_ids'.format(s, len(per_frame), len(ids_per_frame)))
        arrays = [np.asarray(g, np.float64).reshape(-1, LABEL_COLS) for g in per_frame]
        tids = [np.asarray(t, np.int64).reshape(-1) for t in ids_per_frame]
        for k, (g, t) in enumerate(zip(arrays, tids)):
            if g.shape[0] != t.shape[0]:
                raise ValueError('sequence {} frame {}: {} labels, {} track_ids'.format(s, k, g.shape[0], t.shape[0]))
            in_play = t[g[:, 0] <= 1]
            if np.unique(in_play).size != in_play.size:
                raise ValueError('sequence {} frame {}: a track_id labels two objects'.format(s, k))
        cars = np.unique(np.concatenate([t[g[:, 0] == 0] for g, t in zip(arrays, tids)] + [np.zeros(0, np.int64)]))
        traj_ids.append(cars)
        for k in range(frames[s]):
            g = arrays[k] if k < len(arrays) else np.zeros((0, LABEL_COLS))
            t = tids[k] if k < len(tids) else np.zeros(0, np.int64)
            label_list.append(g)
            traj_list.append(np.where(g[:, 0] == 0, np.searchsorted(cars, t), -1).astype(np.int32) if g.shape[0] else np.zeros(0, np.int32))
    packed, counts = kitti_eval.pack_labels(label_list)
    A = packed.shape[1]
    if A > MAX_LABELS:
        raise ValueError('a frame has {} labels, at most {}'.format(A, MAX_LABELS))
    traj = np.full((N, A), -1, np.int32)
    for k, t in enumerate(traj_list):
        traj[k, :t.shape[0]] = t
    # ---- rows
    if on_device:
        import torch
        D = max([int(t[0].shape[1]) for t in tracks] + [1])
        parts_r, parts_i = [], []
        for s, (r, i) in enumerate(tracks):
            if r.dim() != 3 or int(r.shape[2]) != POSE_COLS or tuple(i.shape) != tuple(r.shape[:2]):
                raise ValueError('sequence {}: rows must be (N, D, {}) and ids (N, D), got {} and {}'.format(s, POSE_COLS, tuple(r.shape), tuple(i.shape)))
            n, d = int(r.shape[0]), int(r.shape[1])
            if n == frames[s] and d == D and len(tracks) == 1:
                parts_r.append(r.contiguous())
                parts_i.append(i.to(torch.int32).contiguous())
                continue
            pr = torch.full((frames[s], D, POSE_COLS), -1.0, dtype=torch.float32, device=r.device)
            pi = torch.full((frames[s], D), -1, dtype=torch.int32, device=r.device)
            pr[:n, :d], pi[:n, :d] = r, i
            parts_r.append(pr)
            parts_i.append(pi)
        rows = parts_r[0] if len(parts_r) == 1 else torch.cat(parts_r)
        ids = parts_i[0] if len(parts_i) == 1 else torch.cat(parts_i)
    else:
        per_frame_rows, per_frame_ids = [], []
        for s, (r, i) in enumerate(tracks):
            if _frames_of(r) != _frames_of(i):
                raise ValueError('sequence {}: {} frames of rows, {} of ids'.format(s, _frames_of(r), _frames_of(i)))
            for k in range(frames[s]):
                rk = np.asarray(r[k], np.float32).reshape(-1, POSE_COLS) if k < _frames_of(r) else np.zeros((0, POSE_COLS), np.float32)
                ik = np.asarray(i[k]).reshape(-1).astype(np.int32) if k < _frames_of(r) else np.zeros(0, np.int32)
                if rk.shape[0] != ik.shape[0]:
                    raise ValueError('sequence {} frame {}: {} rows, {} ids'.format(s, k, rk.shape[0], ik.shape[0]))
                live = ik[(rk[:, 14] >= 0) & (ik >= 0)]
                if np.unique(live).size != live.size:
                    raise ValueError('sequence {} frame {}: a tracker id appears twice'.format(s, k))
                per_frame_rows.append(rk)
                per_frame_ids.append(ik)
        D = max([r.shape[0] for r in per_frame_rows] + [1])
        rows = np.full((N, D, POSE_COLS), -1.0, np.float32)
        ids = np.full((N, D), -1, np.int32)
        for k, (rk, ik) in enumerate(zip(per_frame_rows, per_frame_ids)):
            rows[k, :rk.shape[0]], ids[k, :ik.shape[0]] = rk, ik
    if D > MAX_ROWS:
        raise ValueError('a frame has {} rows, at most {}'.format(D, MAX_ROWS))
    return Packed(packed, counts, traj, rows, ids, seq_start, traj_ids)


# ---------------------------------------------------------------------------------------------------- one frame on the host
def label_status(labels, max_occlusion=2.0, max_truncation=0.0, min_height=25.0):
    """ (A, 16) -> (A,) int8: COUNTING, IGNORED, DONTCARE or OUT """
    labels = np.asarray(labels, np.float64).reshape(-1, LABEL_COLS)
    kind, trunc, occ = labels[:, 0], labels[:, 1], labels[:, 2]
    height = np.abs(labels[:, 7] - labels[:, 5])
    hard = (occ > max_occlusion) | (trunc > max_truncation) | (height < min_height)
    return np.where(kind == 0, np.where(hard, IGNORED, COUNTING), np.where(kind == 1, IGNORED, np.where(kind == 2, DONTCARE, OUT))).astype(np.int8)


def cost_matrix_np(overlap, status, live, min_overlap=0.5):
    """ overlap (D, A) float64 -- one plane of the overlaps --, status (A,), live (D,) bool -> (cost (n, n) int64, label_index (G,),
    row_index (T,)): the labels in play are the matrix's rows, the live rows its columns, both in ascending order; n = max(G, T) """
    overlap = np.asarray(overlap, np.float64)
    gl, rl = np.flatnonzero(np.asarray(status) <= IGNORED), np.flatnonzero(live)
    n = max(gl.size, rl.size)
    cost = np.full((n, n), BIG, np.int64)
    if gl.size and rl.size:
        o = overlap[np.ix_(rl, gl)].T                                                   # (G, T)
        with np.errstate(invalid='ignore', over='ignore'):
            admissible = o >= min_overlap                                               # (false for NaN)
            x = np.where(admissible, o, 0.0) * float(SCALE)
            k = np.floor(np.where(x > float(SCALE), float(SCALE), x)).astype(np.int64)
        cost[:gl.size, :rl.size] = np.where(admissible, SCALE - k, BIG)
    return cost, gl, rl


def assign_np(cost):
    """ the optimal assignment of a square int64 matrix by shortest augmenting paths, rows in order, first column on ties (section 4.29,
    operation for operation) -> (column_of_row (n,) int64, total cost) """
    cost = np.asarray(cost, np.int64)
    n = cost.shape[0]
    u, v, p = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for i in range(n):
        minv, way = np.full(n, _INF, np.int64), np.full(n, -1, np.int64)
        used, in_tree = np.zeros(n, bool), np.zeros(n, bool)
        i0, j0 = i, -1
        while True:
            in_tree[i0] = True
            free = ~used
            cur = cost[i0] - u[i0] - v
            better = free & (cur < minv)
            minv[better], way[better] = cur[better], j0
            masked = np.where(free, minv, _INF)
            j1 = int(np.argmin(masked))                                                 # (the first of equals)
            delta = masked[j1]
            v[used] -= delta
            minv[free] -= delta
            u[in_tree] += delta
            j0 = j1
            used[j0] = True
            i0 = int(p[j0])
            if i0 < 0:
                break
        while j0 >= 0:
            j1 = int(way[j0])
            p[j0] = i if j1 < 0 else p[j1]
            j0 = j1
    col = np.empty(n, np.int64)
    col[p] = np.arange(n)
    return col, int(cost[np.arange(n), col].sum()) if n else 0


def frame_np(overlaps, labels, rows, ids, params):
    """ one frame: overlaps (4, D, A), labels (A, 16), rows (D, 36), ids (D,) -> (match (A,) int32, label_outcome (A,) int32, row_outcome
    (D,) int32, counts (8,) int64) """
    labels = np.asarray(labels, np.float64).reshape(-1, LABEL_COLS)
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    ids = np.asarray(ids).reshape(-1)
    D, A = rows.shape[0], labels.shape[0]
    overlaps = np.asarray(overlaps, np.float64).reshape(4, D, A)
    status = label_status(labels, params['max_occlusion'], params['max_truncation'], params['min_height'])
    live = (rows[:, 14] >= 0) & (ids >= 0)
    cost, gl, rl = cost_matrix_np(overlaps[METRICS.index(params['metric'])], status, live, params['min_overlap'])
    col, total = assign_np(cost)
    match, lout, rout = np.full(A, -1, np.int32), np.zeros(A, np.int32), np.zeros(D, np.int32)
    lout[status == COUNTING], lout[status == IGNORED] = L_FN, L_IGNORED_UNMATCHED
    height = np.abs(rows[:, 29].astype(np.float64) - rows[:, 27].astype(np.float64))
    with np.errstate(invalid='ignore'):
        in_stuff = (overlaps[3][:, status == DONTCARE] > 0.5).any(axis=1)
    rout[live] = np.where(height[live] < params['min_height'], R_LOW, np.where(in_stuff[live], R_DONTCARE, R_FP))
    sum_k = 0
    for g in range(gl.size):
        t = int(col[g])
        if t >= rl.size or cost[g, t] >= BIG:                                           # (a pair at BIG is no pair)
            continue
        a, d = gl[g], rl[t]
        match[a] = d
        counting = status[a] == COUNTING
        lout[a], rout[d] = (L_TP, R_TP) if counting else (L_IGNORED_MATCHED, R_IGNORED)
        sum_k += int(SCALE - cost[g, t]) if counting else 0
    counts = np.array([(lout == L_TP).sum(), (rout == R_FP).sum(), (lout == L_FN).sum(), (status == COUNTING).sum(), sum_k, total,
                       gl.size, rl.size], np.int64)
    return match, lout, rout, counts


def clear_np(match, label_outcome, traj, ids, frame_counts, seq_start, n_traj):
    """ the sequence level: match, label_outcome, traj (N, A), ids (N, D), frame_counts (N, 8), n_traj per sequence -> (seq_counts
    (S, 16) int64, [table (n_traj_s, 4) int32: counting frames, matched frames, switches, fragmentations]) """
    S = len(seq_start) - 1
    seq_counts = np.zeros((S, 16), np.int64)
    tables = []
    for s in range(S):
        f0, f1 = int(seq_start[s]), int(seq_start[s + 1])
        table = np.zeros((int(n_traj[s]), 4), np.int32)
        last = np.full(int(n_traj[s]), -1, np.int64)
        before, gap = np.zeros(int(n_traj[s]), bool), np.zeros(int(n_traj[s]), bool)
        for f in range(f0, f1):
            for a in np.flatnonzero((label_outcome[f] == L_TP) | (label_outcome[f] == L_FN)):
                t = int(traj[f, a])
                table[t, 0] += 1
                if label_outcome[f, a] == L_FN:
                    gap[t] = True
                    continue
                track_id = int(ids[f, match[f, a]])
                table[t, 1] += 1
                if before[t]:
                    table[t, 2] += last[t] != track_id
                    table[t, 3] += gap[t]
                last[t], before[t], gap[t] = track_id, True, False
        seq_counts[s, :6] = frame_counts[f0:f1, :6].sum(axis=0)
        seen = table[table[:, 0] > 0].astype(np.int64)
        mt = 5 * seen[:, 1] >= 4 * seen[:, 0]
        ml = 5 * seen[:, 1] < seen[:, 0]
        seq_counts[s, 6:13] = [seen[:, 2].sum(), seen[:, 3].sum(), mt.sum(), (~mt & ~ml).sum(), ml.sum(), seen.shape[0], f1 - f0]
        tables.append(table)
    return seq_counts, tables


# ---------------------------------------------------------------------------------------------------- the summary (both forms)
def summarise(counts):
    """ the 13 integers of SEQ_COUNTS -> a dict of them and the ratios; a ratio without a denominator is None """
    out = {name: int(v) for name, v in zip(SEQ_COUNTS, counts)}
    tp, fp, fn, n_gt = out['tp'], out['fp'], out['fn'], out['n_gt']
    ratio = lambda num, den: (num / den) if den > 0 else None  # noqa: E731
    out['mota'] = None if n_gt == 0 else 1.0 - (fn + fp + out['ids']) / n_gt
    out['motp'] = ratio(out['sum_k'], tp * SCALE)
    out['recall'], out['precision'] = ratio(tp, tp + fn), ratio(tp, tp + fp)
    r, p = out['recall'], out['precision']
    out['f1'] = None if r is None or p is None or r + p == 0 else 2.0 * p * r / (p + r)
    return out


def _result(packed, params, match, lout, rout, frame_counts, seq_counts, tables, names):
    return {'params': dict(params), 'names': list(names) if names is not None else [str(s) for s in range(len(tables))],
            'sequences': [summarise(c[:13]) for c in seq_counts], 'all': summarise(seq_counts[:, :13].sum(axis=0)),
            'trajectories': [{'track_ids': np.asarray(i), 'table': t} for i, t in zip(packed.traj_ids, tables)],
            'frames': {'match': match, 'label_outcome': lout, 'row_outcome': rout, 'counts': frame_counts},
            'seq_start': np.asarray(packed.seq_start)}


def evaluate_packed_np(packed, params, names=None, hota=False, idf1=False):
    """ the NumPy form.  A frame's overlaps are computed once: with hota or idf1 its similarity (utils/pair_tables.similarity_np) is formed
    from them here, behind the frame's codes, and handed to both scores """
    N, A, D = packed.labels.shape[0], packed.labels.shape[1], packed.rows.shape[1]
    match, lout = np.full((N, A), -1, np.int32), np.zeros((N, A), np.int32)
    rout, frame_counts = np.zeros((N, D), np.int32), np.zeros((N, 8), np.int64)
    from . import pair_tables
    plane, similarities = METRICS.index(params['metric']), []
    for f in range(N):
        c = int(packed.label_counts[f])
        o = kitti_eval.image_overlaps(packed.rows[f], packed.labels[f, :c])
        match[f, :c], lout[f, :c], rout[f], frame_counts[f] = frame_np(o, packed.labels[f, :c], packed.rows[f], packed.ids[f], params)
        if hota or idf1:
            similarities.append(pair_tables.similarity_np(o[plane], lout[f, :c], rout[f]))
    seq_counts, tables = clear_np(match, lout, packed.traj, packed.ids, frame_counts, packed.seq_start, [t.size for t in packed.traj_ids])
    result = _result(packed, params, match, lout, rout, frame_counts, seq_counts, tables, names)
    if hota:
        from . import hota_eval
        hota_eval.add_hota_np(result, packed, params, similarities)
    if idf1:
        from . import idf1_eval
        idf1_eval.add_idf1_np(result, packed, params, similarities)
    return result


def evaluate_packed_device(packed, params, names=None, hota=False, idf1=False):
    """ csrc/mot_eval.hip: the frames in chunks whose overlaps stay below utils/kitti_eval.OVERLAP_WORKSPACE_BYTES, one assignment launch
    per chunk, then one launch for all trajectories; rows and ids that are device tensors already are used where they lie.
    hota: csrc/hota_eval.hip beside it (utils/hota_eval.DeviceRun) -- its pass 1 in this sweep over the chunks, its pass 2 in a second
    sweep, which recomputes the overlaps unless the call has a single chunk.
    idf1: csrc/idf1_eval.hip (utils/idf1_eval.DeviceRun) -- its count in this sweep over the chunks, its one assignment after it.
    Both work on one utils/pair_tables.Geometry, built once """
    import torch
    from ..backend import hip
    dev = packed.rows.device if _is_tensor(packed.rows) else hip.require_device()
    n_traj = max([t.size for t in packed.traj_ids] + [0])
    if n_traj > MAX_TRAJECTORIES:
        raise ValueError('a sequence has {} trajectories, the device form takes {}: use device=False'.format(n_traj, MAX_TRAJECTORIES))
    N, A, D = packed.labels.shape[0], packed.labels.shape[1], int(packed.rows.shape[1])
    prm = hip.MotParams(METRICS.index(params['metric']), 0, params['min_overlap'], params['max_occlusion'], params['max_truncation'],
                        params['min_height'])
    rows = packed.rows if _is_tensor(packed.rows) else torch.as_tensor(packed.rows).to(dev, non_blocking=True)
    ids = packed.ids if _is_tensor(packed.ids) else torch.as_tensor(packed.ids).to(dev, non_blocking=True)
    labels = torch.as_tensor(packed.labels).to(dev, non_blocking=True)
    counts = torch.as_tensor(packed.label_counts).to(dev, non_blocking=True)
    traj = torch.as_tensor(packed.traj).to(dev, non_blocking=True)
    step = kitti_eval.chunk_images(D, A)
    hota_run = idf1_run = None
    if hota or idf1:
        from . import pair_tables
        geometry = pair_tables.Geometry(packed, params, rows, ids, traj)
    if hota:
        from . import hota_eval
        hota_run = hota_eval.DeviceRun(geometry, step, rows.device)
    if idf1:
        from . import idf1_eval
        idf1_run = idf1_eval.DeviceRun(geometry, step, rows.device)
    parts = []
    for at in range(0, N, step):
        r, g, c, i = rows[at:at + step], labels[at:at + step], counts[at:at + step], ids[at:at + step]
        overlaps = hip.kitti_overlaps(r, g, c)
        parts.append(hip.mot_assign(overlaps, g, c, r, i, prm))
        if hota_run is not None:
            hota_run.potential(at, overlaps, parts[-1][1], parts[-1][2], keep=N <= step)
        if idf1_run is not None:
            idf1_run.count(at, overlaps, parts[-1][1], parts[-1][2])
        del overlaps
    if parts:
        match, lout, rout, frame_counts = [parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts]) for k in range(4)]
    else:
        match, lout = torch.zeros((0, A), dtype=torch.int32, device=dev), torch.zeros((0, A), dtype=torch.int32, device=dev)
        rout, frame_counts = torch.zeros((0, D), dtype=torch.int32, device=dev), torch.zeros((0, 8), dtype=torch.int64, device=dev)
    seq_counts, table = hip.mot_clear(match, lout, traj, ids, frame_counts, packed.seq_start, n_traj)
    table = table.cpu().numpy()
    tables = [table[s, :t.size].copy() for s, t in enumerate(packed.traj_ids)]
    result = _result(packed, params, match.cpu().numpy(), lout.cpu().numpy(), rout.cpu().numpy(), frame_counts.cpu().numpy(),
                     seq_counts.cpu().numpy(), tables, names)
    if hota_run is not None:
        hota_run.add_to(result, lambda at, n: hip.kitti_overlaps(rows[at:at + n], labels[at:at + n], counts[at:at + n]))
    if idf1_run is not None:
        idf1_run.add_to(result)
    return result


def evaluate_sequences(labels, tracks, metric='image', min_overlap=0.5, device=False, max_occlusion=2.0, max_truncation=0.0,
                       min_height=25.0, names=None, hota=False, idf1=False):
    """ CLEAR-MOT of S sequences.  labels: per sequence (labels_per_frame, track_ids_per_frame); tracks: per sequence (rows, ids) -- see
    the module's text.  Returns {'sequences': [per sequence], 'all': over all sequences, each a dict of the integers tp fp fn n_gt sum_k
    cost ids frag mt pt ml trajectories frames and the ratios mota motp recall precision f1 (None without a denominator);
    'trajectories': per sequence {'track_ids', 'table' (n, 4): counting frames, matched frames, switches, fragmentations};
    'frames': {'match' (N, A), 'label_outcome' (N, A), 'row_outcome' (N, D), 'counts' (N, 8)}; 'names', 'params', 'seq_start'}.
    device=False: NumPy.  device=True: csrc/mot_eval.hip (up to 1024 trajectories per sequence).
    hota=True adds HOTA (utils/hota_eval.py): the key 'hota' in every per-sequence dict and in 'all', and
    'hota_frames' and 'hota_pairs' in the result; without it the result is as described above.
    idf1=True adds the identity scores (utils/idf1_eval.py): the key 'idf1' in every per-sequence dict and in 'all'
    -- {'idf1', 'idr', 'idp', 'integers': {'idtp', 'idfn', 'idfp'}} -- and 'idf1_pairs' in the result, per sequence {'C', 'gc', 'tc',
    'match'}; without it the result is as described above. """
    params = check_params(metric, min_overlap, max_occlusion, max_truncation, min_height)
    packed = pack_sequences(labels, tracks)
    if device:
        return evaluate_packed_device(packed, params, names, hota=hota, idf1=idf1)
    if _is_tensor(packed.rows):
        raise ValueError('device tensors are scored by the device form: device=True')
    return evaluate_packed_np(packed, params, names, hota=hota, idf1=idf1)


def evaluate_tracking(label_path, track_path, **options):
    """ two files -- label_02 lines and the tracker's lines of one sequence -- or two directories: every `.txt` file of the label directory
    is a sequence, scored against the file of the same name in the track directory (a missing file: a sequence without tracks).  The
    options are evaluate_sequences'. """
    if os.path.isdir(label_path) != os.path.isdir(track_path):
        raise ValueError('give two files or two directories')
    if os.path.isdir(label_path):
        names = sorted(f for f in os.listdir(label_path) if f.endswith('.txt'))
        pairs = [(os.path.join(label_path, f), os.path.join(track_path, f)) for f in names]
        names = [os.path.splitext(f)[0] for f in names]
    else:
        names, pairs = [os.path.splitext(os.path.basename(label_path))[0]], [(label_path, track_path)]
    labels = [read_tracking_labels(g) for g, _ in pairs]
    tracks = [read_track_file(t) if os.path.isfile(t) else ([], []) for _, t in pairs]
    return evaluate_sequences(labels, tracks, names=names, **options)


def summary_table(result):
    """ one line per sequence and one for all of them; a result with HOTA (hota=True) has eight more columns, one with the identity
    scores (idf1=True) three more after them """
    def fmt(v, scale=100.0):
        return '   n/a' if v is None else '{:6.2f}'.format(scale * v)

    head = '{:>10s}  MOTA   MOTP   recall prec   F1     TP     FP     FN     IDS   FRAG  MT   PT   ML   GT     frames'.format('sequence')
    with_hota = 'hota' in result['all']
    if with_hota:
        from . import hota_eval
        head += hota_eval.TABLE_HEAD
    with_idf1 = 'idf1' in result['all']
    if with_idf1:
        from . import idf1_eval
        head += idf1_eval.TABLE_HEAD
    lines = [head]
    for name, e in list(zip(result['names'], result['sequences'])) + [('all', result['all'])]:
        lines.append('{:>10s} {} {} {} {} {} {:6d} {:6d} {:6d} {:6d} {:6d} {:4d} {:4d} {:4d} {:6d} {:6d}'.format(
            str(name)[-10:], fmt(e['mota']), fmt(e['motp']), fmt(e['recall']), fmt(e['precision']), fmt(e['f1']), e['tp'], e['fp'], e['fn'],
            e['ids'], e['frag'], e['mt'], e['pt'], e['ml'], e['n_gt'], e['frames']))
        if with_hota:
            lines[-1] += ' ' + hota_eval.table_columns(e)
        if with_idf1:
            lines[-1] += ' ' + idf1_eval.table_columns(e)
    p = result['params']
    also = {(True, False): ' and HOTA', (False, True): ' and Identity', (True, True): ', HOTA and Identity'}.get((with_hota, with_idf1), '')
    return 'CLEAR-MOT{}, Car, {} overlap >= {}\n'.format(also, p['metric'], p['min_overlap']) + '\n'.join(lines)


def result_as_json(result):
    """ the summaries and the trajectory tables with lists, for json.dump (the per-frame codes are left out) """
    return {'params': result['params'], 'all': result['all'],
            'sequences': {str(n): e for n, e in zip(result['names'], result['sequences'])},
            'trajectories': {str(n): {'track_ids': t['track_ids'].tolist(), 'table': t['table'].tolist()}
                             for n, t in zip(result['names'], result['trajectories'])}}
