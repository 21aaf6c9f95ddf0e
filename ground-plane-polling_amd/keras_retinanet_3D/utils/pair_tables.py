"""
The pair tables of a sequence, which HOTA (utils/hota_eval.py) and the identity scores (utils/idf1_eval.py, section
4.31) both fill: a cell per (label trajectory, tracker id) pair and a counter per trajectory and per tracker id.  Here is what the two
share -- a row's tracker index, where a sequence's cells and counters lie (`tables`), how an overlap becomes the similarity of a COUNTING
label (label_outcome 1 or 2) and a KEPT row (row_outcome 1 or 3) (`similarity_np`) --, for the host form (`frames_np`) and the device
form (`Geometry`).  csrc/pair_tables.h is the same decision on the C++ side.
"""
import numpy as np

from . import kitti_eval
from . import mot_eval

SCALE_BITS, SCALE = mot_eval.SCALE_BITS, mot_eval.SCALE
MAX_FRAMES = 1 << 20                        # per sequence: keeps every integer below 2^63
PAIR_TABLE_BYTES = 1 << 30                  # the device form's cap on the pair tables' workspace


# ---------------------------------------------------------------------------------------------------- the tables' geometry
def tracker_index_np(rows, ids, seq_start):
    """ rows (N, D, 36), ids (N, D) -> (trk (N, D) int32: the index of a live row's id among the ids of its sequence, ascending; -1
    otherwise, [n_trk per sequence]) """
    rows, ids = np.asarray(rows), np.asarray(ids)
    live = (rows[:, :, 14] >= 0) & (ids >= 0)
    trk, n_trk = np.full(ids.shape, -1, np.int32), []
    for s in range(len(seq_start) - 1):
        f0, f1 = int(seq_start[s]), int(seq_start[s + 1])
        m = live[f0:f1]
        u, inv = np.unique(ids[f0:f1][m], return_inverse=True)
        trk[f0:f1][m] = inv.astype(np.int32)
        n_trk.append(int(u.size))
    return trk, n_trk


def tracker_index_device(rows, ids, seq_start):
    """ the same with torch ops on device tensors: the ids are not read back, only how many there are """
    import torch
    live = (rows[:, :, 14] >= 0) & (ids >= 0)
    trk, n_trk = torch.full_like(ids, -1), []
    for s in range(len(seq_start) - 1):
        f0, f1 = int(seq_start[s]), int(seq_start[s + 1])
        m = live[f0:f1]
        u, inv = torch.unique(ids[f0:f1][m], sorted=True, return_inverse=True)
        trk[f0:f1][m] = inv.to(torch.int32)
        n_trk.append(int(u.numel()))
    return trk, n_trk


def tables(seq_start, n_gt, n_trk):
    """ -> (seq_tab (S, 6) int32: cell_base, n_gt, n_trk, vec_base, first frame, one past the last; frame_tab (N, 4) int32: a frame's
    line is its sequence's first four; cells; vecs) """
    S = len(seq_start) - 1
    frames = np.diff(np.asarray(seq_start, np.int64))
    if frames.size and int(frames.max()) > MAX_FRAMES:
        raise ValueError('a sequence has {} frames, HOTA takes at most {}'.format(int(frames.max()), MAX_FRAMES))
    n_gt, n_trk = np.asarray(n_gt, np.int64).reshape(S), np.asarray(n_trk, np.int64).reshape(S)
    cell_base = np.concatenate([[0], np.cumsum(n_gt * n_trk)])
    vec_base = np.concatenate([[0], np.cumsum(n_gt + n_trk)])
    seq_tab = np.stack([cell_base[:-1], n_gt, n_trk, vec_base[:-1], np.asarray(seq_start[:-1], np.int64), np.asarray(seq_start[1:], np.int64)],
                       axis=1).reshape(S, 6)
    cells, vecs = int(cell_base[-1]), int(vec_base[-1])
    if max(cells, vecs) >= 1 << 31:
        raise ValueError('pair tables of {} cells: HOTA takes fewer than 2^31'.format(cells))
    seq_tab = seq_tab.astype(np.int32)
    return seq_tab, np.ascontiguousarray(np.repeat(seq_tab[:, :4], frames, axis=0)), cells, vecs


# ---------------------------------------------------------------------------------------------------- the host form
def similarity_np(plane, label_outcome, row_outcome):
    """ plane (D, A) float64 -- one plane of the overlaps --, the frame's codes -> (q (G', T') int64, label_index (G',), row_index (T',)):
    the counting labels are q's rows, the kept rows its columns, both ascending """
    lout, rout = np.asarray(label_outcome), np.asarray(row_outcome)
    gl, rl = np.flatnonzero((lout == 1) | (lout == 2)), np.flatnonzero((rout == 1) | (rout == 3))
    o = np.asarray(plane, np.float64)[np.ix_(rl, gl)].T
    with np.errstate(invalid='ignore', over='ignore'):
        x = np.where(o > 0.0, o, 0.0) * float(SCALE)                                    # (NaN and o <= 0: 0)
        q = np.floor(np.where(x > float(SCALE), float(SCALE), x)).astype(np.int64)
    return q, gl, rl


def frames_np(result, packed, params, similarities=None):
    """ what the host forms of both scores walk: the sequences' geometry and every frame's similarity, from utils/mot_eval's result
    -> (trk (N, D) int32, n_gt and n_trk per sequence, [per frame similarity_np's (q, label_index, row_index)]).
    similarities: that list where the caller has it already (utils/mot_eval.evaluate_packed_np forms it from the overlaps it computes
    anyway); formed here otherwise.  ValueError beyond the limits of `tables`. """
    seq_start = np.asarray(packed.seq_start)
    trk, n_trk = tracker_index_np(packed.rows, packed.ids, seq_start)
    n_gt = [t.size for t in packed.traj_ids]
    tables(seq_start, n_gt, n_trk)                                                      # (the frame limit)
    if similarities is None:
        lout, rout = result['frames']['label_outcome'], result['frames']['row_outcome']
        plane = mot_eval.METRICS.index(params['metric'])
        similarities = []
        for f in range(packed.labels.shape[0]):
            c = int(packed.label_counts[f])
            o = kitti_eval.image_overlaps(packed.rows[f], packed.labels[f, :c])[plane]
            similarities.append(similarity_np(o, lout[f, :c], rout[f]))
    return trk, n_gt, n_trk, similarities


# ---------------------------------------------------------------------------------------------------- the device form
class Geometry(object):
    """ the pair tables of one utils/mot_eval.evaluate_packed_device call, built once and handed to the scores' DeviceRun: trk (N, D) int32
    on the device, n_gt and n_trk per sequence, seq_tab, frame_tab, cells, vecs (`tables`), and metric, the plane of the overlaps """

    def __init__(self, packed, params, rows, ids, traj):
        seq_start = np.asarray(packed.seq_start)
        self.traj, self.metric = traj, mot_eval.METRICS.index(params['metric'])
        self.N, self.S = int(seq_start[-1]), len(seq_start) - 1
        if mot_eval._is_tensor(packed.rows):
            self.trk, self.n_trk = tracker_index_device(rows, ids, seq_start)
        else:
            import torch
            trk, self.n_trk = tracker_index_np(packed.rows, packed.ids, seq_start)
            self.trk = torch.as_tensor(trk).to(rows.device, non_blocking=True)
        self.n_gt = [t.size for t in packed.traj_ids]
        self.seq_tab, self.frame_tab, self.cells, self.vecs = tables(seq_start, self.n_gt, self.n_trk)

    def chunk(self, at, n):
        """ what a frame call of backend/hip.py takes for the frames at .. at + n, between the codes and the workspace: (traj, trk, metric,
        frame_tab, cells, vecs) """
        return self.traj[at:at + n], self.trk[at:at + n], self.metric, self.frame_tab[at:at + n].reshape(-1), self.cells, self.vecs

    def cells_of(self, s, x):
        """ sequence s's part of a downloaded array with a line per cell, x (cells, ...) -> a copy (n_gt, n_trk, ...) """
        cell_base, n_gt, n_trk = (int(v) for v in self.seq_tab[s, :3])
        return x[cell_base:cell_base + n_gt * n_trk].reshape((n_gt, n_trk) + x.shape[1:]).copy()

    def counters_of(self, s, x):
        """ sequence s's parts of a downloaded array with an entry per counter, x (vecs,) -> copies (its trajectories' (n_gt,), its
        tracker ids' (n_trk,)) """
        n_gt, n_trk, vec_base = (int(v) for v in self.seq_tab[s, 1:4])
        return x[vec_base:vec_base + n_gt].copy(), x[vec_base + n_gt:vec_base + n_gt + n_trk].copy()
