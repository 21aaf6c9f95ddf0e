"""
HOTA scoring of tracks for the class Car: the alignment score of every (label trajectory, tracker id) pair of a sequence, per frame the
optimal assignment on costs that this score weighs, then detection, association and localisation accuracy at the 19 thresholds
0.05 .. 0.95 and their means -- DESIGN.md section 4.30 is the specification.  Parity with TrackEval's hota.py and its KITTI preprocessing
is UNPINNED (TrackEval is not part of this repository).  include/gpp.h (gpp_hota_potential, gpp_hota_match, gpp_hota_reduce) is the device
form's contract.

HOTA starts where utils/mot_eval.py's assignment ends: that assignment, with the call's metric and limits, is the preprocessing.  A label
COUNTS iff its label_outcome is 1 or 2, a row is KEPT iff its row_outcome is 1 or 3; the tables' geometry and the similarity are
utils/pair_tables.py's, shared with utils/idf1_eval.py.  Everything after the similarity q = floor(min(overlap * 2^20, 2^20)) is exact
integers, so the two forms and the loop-written oracle of the tests are equal with ==:

    device=False    NumPy: potential_np (pass 1), align_np, match_np (pass 2, on utils/mot_eval.assign_np), reduce_np.
    device=True     csrc/hota_eval.hip: per chunk of frames gpp_hota_potential in a first sweep, gpp_hota_match in a second one -- pass 1
                    must have seen every frame of a sequence before pass 2 sees any --, then gpp_hota_reduce.
Both end in the same host code (summarise_hota), fed with the same integers.
"""
import math

import numpy as np

from . import mot_eval
from . import pair_tables

SCALE_BITS, SCALE = mot_eval.SCALE_BITS, mot_eval.SCALE
LEVELS = 19                                 # GPP_HOTA_LEVELS: the thresholds j / 20, j = 1 .. 19
HIST = 20                                   # GPP_HOTA_HIST: a cell's counters, index jm (0 unused)
FRAME_COLS = 40                             # GPP_HOTA_FRAME_COLS: TP_1..19, SQ_1..19, G', T'
SEQ_COLS = 8                                # GPP_HOTA_SEQ_COLS
SEQ_INTEGERS = ('tp', 'fn', 'fp', 'sq', 'ass', 'assre', 'asspr')
RATIOS = ('hota', 'deta', 'assa', 'detre', 'detpr', 'assre', 'asspr', 'loca')


# ---------------------------------------------------------------------------------------------------- one frame on the host
def potential_np(q, g, t, P, gc, tc):
    """ pass 1 of one frame, in place: q (G', T') int64 -- utils/pair_tables.similarity_np's --, g (G',) the labels' trajectories, t (T',)
    the rows' tracker indices; P (n_gt, n_trk) int64, gc (n_gt,) and tc (n_trk,) int32 are the sequence's """
    q = np.asarray(q, np.int64)
    rs, cs = q.sum(axis=1, keepdims=True), q.sum(axis=0, keepdims=True)
    den = np.where(q > 0, rs + cs - q, 1)
    p = np.where(q > 0, (q << SCALE_BITS) // den, 0)
    np.add.at(P, (np.asarray(g)[:, None], np.asarray(t)[None, :]), p)
    np.add.at(gc, g, 1)
    np.add.at(tc, t, 1)


def align_np(P, gc, tc):
    """ the alignment score A (n_gt, n_trk) int32 = floor(P 2^20 / ((gc + tc) 2^20 - P)) where P > 0, else 0 """
    P = np.asarray(P, np.int64)
    den = ((np.asarray(gc, np.int64)[:, None] + np.asarray(tc, np.int64)[None, :]) << SCALE_BITS) - P
    return np.where(P > 0, (P << SCALE_BITS) // np.where(P > 0, den, 1), 0).astype(np.int32)


def cost_np(q, align):
    """ pass 2's square matrix: q (G', T'), align (G', T') -- A of the frame's pairs -- -> (n, n) int64 """
    G, T = q.shape
    n = max(G, T)
    cost = np.full((n, n), SCALE, np.int64)
    cost[:G, :T] = SCALE - ((np.asarray(align, np.int64) * q) >> SCALE_BITS)
    return cost


def match_np(q, align):
    """ pass 2 of one frame -> (pairs (k, 2) int64: (matrix row, matrix column) of the real pairs with jm >= 1, jm (k,) int64, cost) """
    cost = cost_np(q, align)
    G, T = q.shape
    col, _ = mot_eval.assign_np(cost)
    rows = np.array([i for i in range(G) if col[i] < T], np.int64)
    cols = col[rows].astype(np.int64) if rows.size else np.zeros(0, np.int64)
    jm = np.minimum(LEVELS, (20 * q[rows, cols] + 19) >> SCALE_BITS) if rows.size else np.zeros(0, np.int64)
    keep = jm >= 1
    return np.stack([rows[keep], cols[keep]], axis=1).reshape(-1, 2), jm[keep], cost


def reduce_np(hist, gc, tc, frame_hota):
    """ hist (n_gt, n_trk, 20) int32, gc, tc, the sequence's frame_hota (F, 40) int64 -> (19, 8) int64: TP FN FP SQ ASS ASSRE ASSPR 0 """
    out = np.zeros((LEVELS, SEQ_COLS), np.int64)
    frame_hota = np.asarray(frame_hota, np.int64).reshape(-1, FRAME_COLS)
    sums = frame_hota.sum(axis=0)
    out[:, 0], out[:, 3] = sums[:LEVELS], sums[LEVELS:2 * LEVELS]
    out[:, 1], out[:, 2] = sums[2 * LEVELS] - out[:, 0], sums[2 * LEVELS + 1] - out[:, 0]
    mc = np.cumsum(np.asarray(hist, np.int64)[:, :, ::-1], axis=2)[:, :, ::-1]          # mc[..., j]: the sum over m >= j
    g = np.asarray(gc, np.int64)[:, None]
    t = np.asarray(tc, np.int64)[None, :]
    for j in range(1, LEVELS + 1):
        m = mc[:, :, j]
        on = m > 0
        num = (m * m) << SCALE_BITS
        out[j - 1, 4] = (num // np.where(on, g + t - m, 1))[on].sum()
        out[j - 1, 5] = (num // np.where(on, g + np.zeros_like(t), 1))[on].sum()
        out[j - 1, 6] = (num // np.where(on, t + np.zeros_like(g), 1))[on].sum()
    return out


# ---------------------------------------------------------------------------------------------------- the summary (both forms)
def summarise_hota(counts):
    """ (19, 8) integers -> {'integers': {tp fn fp sq ass assre asspr: 19 ints}, 'thresholds': {ratio: 19 floats}, and the eight means
    hota deta assa detre detpr assre asspr loca}.  A zero denominator gives 0.0, for loca 1.0; without a counting label and without a
    kept row every ratio is None.  The square root is taken here, on the host. """
    counts = np.asarray(counts, np.int64).reshape(LEVELS, SEQ_COLS)
    ints = {name: [int(v) for v in counts[:, k]] for k, name in enumerate(SEQ_INTEGERS)}
    out = {'integers': ints}
    if ints['tp'][0] + ints['fn'][0] == 0 and ints['tp'][0] + ints['fp'][0] == 0:
        out['thresholds'] = {name: [None] * LEVELS for name in RATIOS}
        out.update({name: None for name in RATIOS})
        return out
    ratio = lambda num, den, empty=0.0: (num / den) if den > 0 else empty  # noqa: E731
    per = {name: [] for name in RATIOS}
    for j in range(LEVELS):
        tp, fn, fp = ints['tp'][j], ints['fn'][j], ints['fp'][j]
        per['deta'].append(ratio(tp, tp + fn + fp))
        per['detre'].append(ratio(tp, tp + fn))
        per['detpr'].append(ratio(tp, tp + fp))
        per['assa'].append(ratio(ints['ass'][j], SCALE * tp))
        per['assre'].append(ratio(ints['assre'][j], SCALE * tp))
        per['asspr'].append(ratio(ints['asspr'][j], SCALE * tp))
        per['loca'].append(ratio(ints['sq'][j], SCALE * tp, 1.0))
        per['hota'].append(math.sqrt(per['deta'][-1] * per['assa'][-1]))
    out['thresholds'] = per
    out.update({name: sum(per[name]) / LEVELS for name in RATIOS})
    return out


def _add(result, match, frame_hota, seq_hota, pairs):
    for s, e in enumerate(result['sequences']):
        e['hota'] = summarise_hota(seq_hota[s])
    result['all']['hota'] = summarise_hota(seq_hota.sum(axis=0) if seq_hota.shape[0] else np.zeros((LEVELS, SEQ_COLS), np.int64))
    result['hota_frames'] = {'match': match, 'counts': frame_hota}
    result['hota_pairs'] = pairs
    return result


# ---------------------------------------------------------------------------------------------------- the host form
def add_hota_np(result, packed, params, similarities=None):
    """ the NumPy form: adds 'hota' to every summary of utils/mot_eval's result and 'hota_frames' {'match' (N, A) int32, 'counts' (N, 40)
    int64} and 'hota_pairs' [per sequence {'P' int64, 'A' int32 (n_gt, n_trk), 'hist' int32 (n_gt, n_trk, 20), 'gc', 'tc' int32}].
    similarities: the frames' utils/pair_tables.similarity_np where the caller has them; formed here otherwise """
    N, A = packed.labels.shape[0], packed.labels.shape[1]
    seq_start = np.asarray(packed.seq_start)
    S = len(seq_start) - 1
    trk, n_gt, n_trk, frames = pair_tables.frames_np(result, packed, params, similarities)
    match, frame_hota = np.full((N, A), -1, np.int32), np.zeros((N, FRAME_COLS), np.int64)
    seq_hota, pairs = np.zeros((S, LEVELS, SEQ_COLS), np.int64), []
    for s in range(S):
        f0, f1 = int(seq_start[s]), int(seq_start[s + 1])
        P = np.zeros((n_gt[s], n_trk[s]), np.int64)
        gc, tc = np.zeros(n_gt[s], np.int32), np.zeros(n_trk[s], np.int32)
        hist = np.zeros((n_gt[s], n_trk[s], HIST), np.int32)
        for f in range(f0, f1):
            q, gl, rl = frames[f]
            potential_np(q, packed.traj[f, gl], trk[f, rl], P, gc, tc)
        align = align_np(P, gc, tc)
        for f in range(f0, f1):
            q, gl, rl = frames[f]
            g, t = packed.traj[f, gl], trk[f, rl]
            found, jm, _ = match_np(q, align[np.ix_(g, t)])
            for (i, j), m in zip(found, jm):
                match[f, gl[i]] = rl[j]
                hist[g[i], t[j], m] += 1
                frame_hota[f, :m] += 1
                frame_hota[f, LEVELS:LEVELS + m] += q[i, j]
            frame_hota[f, 2 * LEVELS:] = gl.size, rl.size
        seq_hota[s] = reduce_np(hist, gc, tc, frame_hota[f0:f1])
        pairs.append({'P': P, 'A': align, 'hist': hist, 'gc': gc, 'tc': tc})
    return _add(result, match, frame_hota, seq_hota, pairs)


# ---------------------------------------------------------------------------------------------------- the device form
class DeviceRun(object):
    """ csrc/hota_eval.hip beside utils/mot_eval.evaluate_packed_device's walk over the chunks: potential() in the first sweep, finish()
    runs the second sweep and the reduction.  geo: the call's utils/pair_tables.Geometry """

    def __init__(self, geo, step, device):
        from ..backend import hip
        self.hip, self.geo = hip, geo
        need = 92 * geo.cells + 4 * geo.vecs                                            # (before any library call: P, A, hist, the counters)
        if need > pair_tables.PAIR_TABLE_BYTES or geo.cells >= 1 << 31:
            raise ValueError('the pair tables of {} cells need {} bytes, the device form takes {}: use device=False'.format(
                geo.cells, need, pair_tables.PAIR_TABLE_BYTES))
        self.workspace = hip.hota_workspace(geo.cells, geo.vecs, min(step, geo.N), geo.S, device)
        self.codes, self.kept = [], None

    def potential(self, at, overlaps, label_outcome, row_outcome, keep):
        """ pass 1 of the chunk that starts at frame `at`; keep: the call has a single chunk, its overlaps serve pass 2 """
        self.hip.hota_potential(overlaps, label_outcome, row_outcome, *self.geo.chunk(at, int(overlaps.shape[0])), self.workspace)
        self.codes.append((at, label_outcome, row_outcome))
        self.kept = overlaps if keep else None

    def finish(self, overlaps_of):
        """ pass 2 over the chunks -- overlaps_of(at, n) recomputes a chunk's overlaps --, then the reduction
        -> (match (N, A) int32, frame_hota (N, 40) int64, seq_hota (S, 19, 8) int64) on the device """
        import torch
        hip, geo, parts = self.hip, self.geo, []
        for at, lout, rout in self.codes:
            n = int(lout.shape[0])
            overlaps = self.kept if self.kept is not None else overlaps_of(at, n)
            parts.append(hip.hota_match(overlaps, lout, rout, *geo.chunk(at, n), self.workspace))
        dev = self.workspace.device
        if parts:
            match, frame_hota = [parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts]) for k in range(2)]
        else:
            match = torch.zeros((0, int(geo.traj.shape[1])), dtype=torch.int32, device=dev)
            frame_hota = torch.zeros((0, FRAME_COLS), dtype=torch.int64, device=dev)
        seq_hota = hip.hota_reduce(frame_hota, geo.seq_tab.reshape(-1), geo.cells, geo.vecs, self.workspace)
        return match, frame_hota, seq_hota

    def pairs(self):
        """ the pair tables, downloaded: [per sequence {'P', 'A', 'hist', 'gc', 'tc'}] """
        geo = self.geo
        P, align, hist, cnt = [t.cpu().numpy() for t in self.hip.hota_tables(self.workspace, geo.cells, geo.vecs)]
        out = []
        for s in range(geo.S):
            gc, tc = geo.counters_of(s, cnt)
            out.append({'P': geo.cells_of(s, P), 'A': geo.cells_of(s, align), 'hist': geo.cells_of(s, hist), 'gc': gc, 'tc': tc})
        return out

    def add_to(self, result, overlaps_of):
        match, frame_hota, seq_hota = self.finish(overlaps_of)
        return _add(result, match.cpu().numpy(), frame_hota.cpu().numpy(), seq_hota.cpu().numpy(), self.pairs())


# ---------------------------------------------------------------------------------------------------- the entry point and the table
def evaluate_hota_sequences(labels, tracks, metric='image', device=False, **options):
    """ utils/mot_eval.evaluate_sequences with hota=True: its result, with 'hota' in every summary and 'hota_frames' and 'hota_pairs' """
    return mot_eval.evaluate_sequences(labels, tracks, metric=metric, device=device, hota=True, **options)


def table_columns(entry):
    """ the eight columns that --hota adds to a line of utils/mot_eval.summary_table """
    h = entry['hota']
    return ' '.join('   n/a' if h[name] is None else '{:6.2f}'.format(100.0 * h[name]) for name in RATIOS)


TABLE_HEAD = '  HOTA   DetA   AssA   DetRe  DetPr  AssRe  AssPr  LocA'
