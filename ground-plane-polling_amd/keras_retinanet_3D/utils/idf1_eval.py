"""
Identity scoring of tracks for the class Car -- IDF1, IDR, IDP: per sequence the table C of how often every (label trajectory, tracker id)
pair overlaps by at least one half, then ONE optimal assignment per sequence of the trajectories to the tracker ids on that table, and
what it explains (IDTP) against what it leaves (IDFN, IDFP) -- DESIGN.md section 4.31 is the specification.  Parity with TrackEval's
identity.py is UNPINNED (TrackEval is not part of this repository).  include/gpp.h (gpp_idf1_count, gpp_idf1_assign) is the device form's
contract.

The inputs are HOTA's: utils/mot_eval.py's assignment, with the call's metric and limits, is the
preprocessing.  A label COUNTS iff its label_outcome is 1 or 2, a row is KEPT iff its row_outcome is 1 or 3; the tables' geometry and
the similarity are utils/pair_tables.py's.  Everything after q = floor(min(overlap * 2^20, 2^20)) is exact integers, so the two forms and
the loop-written oracle of the tests are equal with ==:

    device=False    NumPy: count_np (pass 1), assign_table_np (pass 2: section 4.29's rule on a rectangular matrix, vectorised over the
                    columns and serial over the steps).
    device=True     csrc/idf1_eval.hip: gpp_idf1_count per chunk of frames in utils/mot_eval.evaluate_packed_device's one sweep (beside
                    gpp_hota_potential when HOTA is scored too), then gpp_idf1_assign once.  The overlaps are never computed again.
Both end in the same host code (summarise_idf1), fed with the same integers.
"""
import numpy as np

from . import mot_eval
from . import pair_tables

SCALE_BITS, SCALE = mot_eval.SCALE_BITS, mot_eval.SCALE
HALF = SCALE >> 1                           # q >= 2^19 is overlap >= 0.5: the scaling is exact
MAX_TRAJECTORIES = mot_eval.MAX_TRAJECTORIES                                            # GPP_MOT_MAX_TRAJECTORIES: the matrix's rows
MAX_IDS = 4096                              # GPP_IDF1_MAX_IDS: the matrix's columns, max(trajectories, tracker ids)
SEQ_COLS = 8                                # GPP_IDF1_SEQ_COLS: IDTP IDFN IDFP sum-gc sum-tc cost G T
SEQ_INTEGERS = ('idtp', 'idfn', 'idfp')
RATIOS = ('idf1', 'idr', 'idp')
_INF = np.iinfo(np.int64).max


def check_sides(n_gt, n_trk):
    """ ValueError beyond the limits of both forms: more than 1024 trajectories, more than 4096 columns """
    n_gt, n_trk = int(n_gt), int(n_trk)
    if n_gt > MAX_TRAJECTORIES:
        raise ValueError('a sequence has {} trajectories, IDF1 takes at most {}'.format(n_gt, MAX_TRAJECTORIES))
    if max(n_gt, n_trk) > MAX_IDS:
        raise ValueError('a sequence has {} tracker ids, IDF1 takes at most {}'.format(n_trk, MAX_IDS))


# ---------------------------------------------------------------------------------------------------- the two passes on the host
def count_np(q, g, t, C, gc, tc):
    """ pass 1 of one frame, in place: q (G', T') int64 -- utils/pair_tables.similarity_np's --, g (G',) the labels' trajectories, t (T',)
    the rows' tracker indices; C (n_gt, n_trk), gc (n_gt,) and tc (n_trk,) int32 are the sequence's.  A label may count with two rows. """
    np.add.at(C, (np.asarray(g)[:, None], np.asarray(t)[None, :]), (np.asarray(q, np.int64) >= HALF).astype(C.dtype))
    np.add.at(gc, g, 1)
    np.add.at(tc, t, 1)


def assign_table_np(C, stats=None):
    """ pass 2: C (G, T) counts -> (id_match (G,) int32: a trajectory's tracker index, -1 for none; IDTP; the assignment's total cost).
    The matrix is G x n, n = max(G, T): 2^20 - C, 2^20 in the padding columns.  Section 4.29's rule for the rows 0 .. G - 1 in order:
    u = v = 0, strict < in the relaxation, the first column on ties, the rows handed back along way.
    stats: a dict that receives 'steps', the number of dependent steps (tools/bench_idf1.py divides the kernel's time by it). """
    C = np.asarray(C)
    if C.ndim != 2:
        raise ValueError('the table must be (trajectories, tracker ids), got {}'.format(C.shape))
    G, T = C.shape
    check_sides(G, T)
    n = max(G, T)
    cost = np.full((G, n), SCALE, np.int64)
    cost[:, :T] -= C.astype(np.int64)
    u, v, p = np.zeros(G, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    steps = 0
    for i in range(G):
        minv, way = np.full(n, _INF, np.int64), np.full(n, -1, np.int64)
        used, in_tree = np.zeros(n, bool), np.zeros(G, bool)
        i0, j0 = i, -1
        while True:
            steps += 1
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
    if stats is not None:
        stats['steps'] = steps
    match = np.full(G, -1, np.int32)
    held = np.flatnonzero(p[:T] >= 0)                                                   # (a padding column explains nothing)
    real = held[C[p[held], held] > 0]
    match[p[real]] = real.astype(np.int32)
    idtp = int(C[p[real], real].astype(np.int64).sum())
    return match, idtp, G * SCALE - idtp


def seq_counts_np(C, gc, tc):
    """ one sequence -> (id_match (G,) int32, the line of seq_idf1 (8,) int64: IDTP IDFN IDFP sum-gc sum-tc cost G T) """
    match, idtp, cost = assign_table_np(C)
    n_g, n_t = int(np.asarray(gc, np.int64).sum()), int(np.asarray(tc, np.int64).sum())
    return match, np.array([idtp, n_g - idtp, n_t - idtp, n_g, n_t, cost, C.shape[0], C.shape[1]], np.int64)


# ---------------------------------------------------------------------------------------------------- the summary (both forms)
def summarise_idf1(counts):
    """ IDTP, IDFN, IDFP (the first three of a seq_idf1 line) -> {'idf1', 'idr', 'idp', 'integers': {'idtp', 'idfn', 'idfp'}}.  A zero
    denominator gives 0.0; without a counting label and without a kept row every ratio is None. """
    idtp, idfn, idfp = (int(v) for v in np.asarray(counts).reshape(-1)[:3])
    out = {'integers': {'idtp': idtp, 'idfn': idfn, 'idfp': idfp}}
    if idtp + idfn == 0 and idtp + idfp == 0:
        out.update({name: None for name in RATIOS})
        return out
    ratio = lambda num, den: (num / den) if den > 0 else 0.0  # noqa: E731
    out['idr'], out['idp'] = ratio(idtp, idtp + idfn), ratio(idtp, idtp + idfp)
    out['idf1'] = ratio(2 * idtp, 2 * idtp + idfn + idfp)
    return out


def _add(result, seq_idf1, pairs):
    seq_idf1 = np.asarray(seq_idf1, np.int64).reshape(-1, SEQ_COLS)
    for s, e in enumerate(result['sequences']):
        e['idf1'] = summarise_idf1(seq_idf1[s])
    result['all']['idf1'] = summarise_idf1(seq_idf1[:, :3].sum(axis=0))
    result['idf1_pairs'] = pairs
    return result


# ---------------------------------------------------------------------------------------------------- the host form
def add_idf1_np(result, packed, params, similarities=None):
    """ the NumPy form: adds 'idf1' to every summary of utils/mot_eval's result and 'idf1_pairs' [per sequence {'C' (n_gt, n_trk), 'gc'
    (n_gt,), 'tc' (n_trk,), 'match' (n_gt,), all int32}].
    similarities: the frames' utils/pair_tables.similarity_np where the caller has them; formed here otherwise """
    seq_start = np.asarray(packed.seq_start)
    S = len(seq_start) - 1
    trk, n_gt, n_trk, frames = pair_tables.frames_np(result, packed, params, similarities)
    for s in range(S):
        check_sides(n_gt[s], n_trk[s])
    seq_idf1, pairs = np.zeros((S, SEQ_COLS), np.int64), []
    for s in range(S):
        C = np.zeros((n_gt[s], n_trk[s]), np.int32)
        gc, tc = np.zeros(n_gt[s], np.int32), np.zeros(n_trk[s], np.int32)
        for f in range(int(seq_start[s]), int(seq_start[s + 1])):
            q, gl, rl = frames[f]
            count_np(q, packed.traj[f, gl], trk[f, rl], C, gc, tc)
        match, seq_idf1[s] = seq_counts_np(C, gc, tc)
        pairs.append({'C': C, 'gc': gc, 'tc': tc, 'match': match})
    return _add(result, seq_idf1, pairs)


# ---------------------------------------------------------------------------------------------------- the device form
class DeviceRun(object):
    """ csrc/idf1_eval.hip beside utils/mot_eval.evaluate_packed_device's walk over the chunks: count() in the one sweep, add_to() runs the
    assignment.  geo: the call's utils/pair_tables.Geometry, which HOTA's run of the same call works on too """

    def __init__(self, geo, step, device):
        from ..backend import hip
        self.hip, self.geo = hip, geo
        for g, t in zip(geo.n_gt, geo.n_trk):
            check_sides(g, t)
        need = 4 * geo.cells + 4 * geo.vecs                                             # (before any library call: C and the counters)
        if need > pair_tables.PAIR_TABLE_BYTES:
            raise ValueError('the tables of {} cells need {} bytes, the device form takes {}: use device=False'.format(
                geo.cells, need, pair_tables.PAIR_TABLE_BYTES))
        self.workspace = hip.idf1_workspace(geo.cells, geo.vecs, min(step, geo.N), geo.S, device)

    def count(self, at, overlaps, label_outcome, row_outcome):
        """ pass 1 of the chunk that starts at frame `at` """
        self.hip.idf1_count(overlaps, label_outcome, row_outcome, *self.geo.chunk(at, int(overlaps.shape[0])), self.workspace)

    def finish(self):
        """ pass 2, after the sweep -> (id_match (vecs,) int32, seq_idf1 (S, 8) int64) on the device """
        return self.hip.idf1_assign(self.geo.seq_tab.reshape(-1), self.geo.cells, self.geo.vecs, self.workspace)

    def add_to(self, result):
        geo = self.geo
        id_match, seq_idf1 = self.finish()
        C, cnt = [t.cpu().numpy() for t in self.hip.idf1_tables(self.workspace, geo.cells, geo.vecs)]
        id_match, pairs = id_match.cpu().numpy(), []
        for s in range(geo.S):
            gc, tc = geo.counters_of(s, cnt)
            pairs.append({'C': geo.cells_of(s, C), 'gc': gc, 'tc': tc, 'match': geo.counters_of(s, id_match)[0]})
        return _add(result, seq_idf1.cpu().numpy(), pairs)


# ---------------------------------------------------------------------------------------------------- the entry point and the table
def evaluate_idf1_sequences(labels, tracks, metric='image', device=False, **options):
    """ utils/mot_eval.evaluate_sequences with idf1=True: its result, with 'idf1' in every summary and 'idf1_pairs' """
    return mot_eval.evaluate_sequences(labels, tracks, metric=metric, device=device, idf1=True, **options)


def table_columns(entry):
    """ the three columns that --idf1 adds to a line of utils/mot_eval.summary_table """
    h = entry['idf1']
    return ' '.join('   n/a' if h[name] is None else '{:6.2f}'.format(100.0 * h[name]) for name in RATIOS)


TABLE_HEAD = '  IDF1   IDR    IDP'
