""" A loop-written oracle of the identity scores in Python integers over dicts, a restatement of the metric's
DEFINITION -- float overlaps, o >= 0.5, the (G + T) x (G + T) matrix with its large constant, scipy's assignment --, and the written
tables the IDF1 tests share.  Nothing here is imported from utils/idf1_eval.py.  The preprocessing -- which labels count, which rows are
kept -- and the overlaps are tests/hota_oracle.prepared's (sections 4.29 and 4.30), which their own tests pin. """
import numpy as np

import hota_oracle as HO

S = 1 << 20
HALF = 1 << 19


# ---------------------------------------------------------------------------------------------------- the rules, in loops and integers
def assign_rows(cost):
    """ cost: G lists of n Python ints, G <= n -> the column of every row.  The textbook 1-based form of the shortest-augmenting-path
    method on a rectangular matrix, with a virtual column 0: rows in order, strict <, the first column on ties """
    G = len(cost)
    n = len(cost[0]) if G else 0
    assert all(len(line) == n for line in cost) and G <= n
    INF = 1 << 62
    u, v, p, way = [0] * (G + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    for i in range(1, G + 1):
        p[0] = i
        j0 = 0
        minv, used = [INF] * (n + 1), [False] * (n + 1)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, 0
            for j in range(1, n + 1):
                if used[j]:
                    continue
                cur = cost[i0 - 1][j - 1] - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            for j in range(n + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = [0] * G
    for j in range(1, n + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def table_scores(C, G, T):
    """ C: {(g, t): count} over 0 <= g < G, 0 <= t < T -> (match [G]: the column or -1, IDTP, the assignment's total cost) """
    n = max(G, T)
    cost = [[S - C.get((g, t), 0) if t < T else S for t in range(n)] for g in range(G)]
    col = assign_rows(cost)
    match = [col[g] if col[g] < T and C.get((g, col[g]), 0) > 0 else -1 for g in range(G)]
    idtp = sum(C[g, match[g]] for g in range(G) if match[g] >= 0)
    assert sum(cost[g][col[g]] for g in range(G)) == G * S - idtp
    return match, idtp, G * S - idtp


def sequence_ids(labels, tracks):
    """ per sequence (the track_ids of its Car labels, the ids of its live rows), both ascending: the tables' rows and columns """
    out = []
    for (lab, tids), (rows, ids) in zip(labels, tracks):
        cars = sorted({int(t) for g, tt in zip(lab, tids) for x, t in zip(np.asarray(g, np.float64).reshape(-1, 16), np.asarray(tt).reshape(-1))
                       if x[0] == 0})
        live = sorted({int(i) for r, ii in zip(rows, ids) for x, i in zip(np.asarray(r).reshape(-1, 36), np.asarray(ii).reshape(-1))
                       if x[14] >= 0 and i >= 0})
        out.append((cars, live))
    return out


def evaluate(labels, tracks, metric='image', **limits):
    """ -> per sequence {'C': {(track_id, tracker id): n > 0}, 'gc', 'tc': {id: n}, 'match': {track_id: tracker id or None}, 'idtp', 'idfn',
    'idfp', 'cost', 'G', 'T'} """
    out = []
    for frames, (cars, live) in zip(HO.prepared(labels, tracks, metric, **limits), sequence_ids(labels, tracks)):
        gi, ti = {g: k for k, g in enumerate(cars)}, {t: k for k, t in enumerate(live)}
        C, gc, tc = {}, {}, {}
        for fr in frames:
            for a, g in fr['labels']:
                gc[g] = gc.get(g, 0) + 1
            for d, t in fr['rows']:
                tc[t] = tc.get(t, 0) + 1
            for a, g in fr['labels']:
                for d, t in fr['rows']:
                    if HO.similarity(fr['o'][a, d]) >= HALF:
                        C[gi[g], ti[t]] = C.get((gi[g], ti[t]), 0) + 1
        match, idtp, cost = table_scores(C, len(cars), len(live))
        n_g, n_t = sum(gc.values()), sum(tc.values())
        out.append({'C': {(cars[g], live[t]): n for (g, t), n in C.items()}, 'gc': gc, 'tc': tc,
                    'match': {cars[g]: (live[m] if m >= 0 else None) for g, m in enumerate(match)},
                    'idtp': idtp, 'idfn': n_g - idtp, 'idfp': n_t - idtp, 'cost': cost, 'G': len(cars), 'T': len(live)})
    return out


# ---------------------------------------------------------------------------------------------------- the definition
def definition_counts(C, gc, tc):
    """ the identity metric as it is defined (Ristani et al., ECCV 2016 workshops; TrackEval's identity.py): C (G, T) the frames in which a
    trajectory and an id overlap, gc (G,) and tc (T,) the frames each is seen in -> (IDTP, IDFN, IDFP).  The (G + T) x (G + T) matrices of
    false negatives and false positives: gc - C / tc - C in the real block, a trajectory's or an id's own count on its "unmatched"
    diagonal, 1e10 elsewhere off the real block, 0 in the block of the unmatched with the unmatched """
    from scipy.optimize import linear_sum_assignment
    C, gc, tc = np.asarray(C, np.float64), np.asarray(gc, np.float64), np.asarray(tc, np.float64)
    G, T = C.shape
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fp[G:, :T] = fn[:G, T:] = 1e10
    for g in range(G):
        fn[g, :T], fn[g, T + g] = gc[g] - C[g], gc[g]
    for t in range(T):
        fp[:G, t], fp[G + t, t] = tc[t] - C[:, t], tc[t]
    ri, ci = linear_sum_assignment(fn + fp)
    idfn, idfp = int(round(fn[ri, ci].sum())), int(round(fp[ri, ci].sum()))
    return int(round(gc.sum())) - idfn, idfn, idfp


def float_identity(labels, tracks, metric='image', **limits):
    """ the definition on the same preprocessing, with the overlaps as floats: per sequence (IDTP, IDFN, IDFP) """
    out = []
    for frames in HO.prepared(labels, tracks, metric, **limits):
        gts = sorted({g for fr in frames for _, g in fr['labels']})
        trs = sorted({t for fr in frames for _, t in fr['rows']})
        gi, ti = {g: k for k, g in enumerate(gts)}, {t: k for k, t in enumerate(trs)}
        C, gc, tc = np.zeros((len(gts), len(trs))), np.zeros(len(gts)), np.zeros(len(trs))
        for fr in frames:
            for a, g in fr['labels']:
                gc[gi[g]] += 1
                for d, t in fr['rows']:
                    if fr['o'][a, d] >= 0.5:
                        C[gi[g], ti[t]] += 1
            for d, t in fr['rows']:
                tc[ti[t]] += 1
        out.append(definition_counts(C, gc, tc))
    return out


def rectangular_total(C):
    """ scipy's optimum on the kernel's own rectangular matrix: G x max(G, T), 2^20 - C and 2^20 in the padding columns """
    from scipy.optimize import linear_sum_assignment
    C = np.asarray(C, np.int64)
    G, T = C.shape
    cost = np.full((G, max(G, T)), S, np.int64)
    cost[:, :T] -= C
    ri, ci = linear_sum_assignment(cost)
    return int(cost[ri, ci].sum())


# ---------------------------------------------------------------------------------------------------- written tables
def sparse_table(seed, G, T, per_row=4, pool=None):
    """ G x T int32 counts with at most `per_row` non-zero cells per row, their columns drawn from the first `pool` columns (default: all):
    a small pool makes the trajectories compete for the same ids """
    rng = np.random.default_rng(seed)
    C = np.zeros((G, T), np.int32)
    pool = T if pool is None else min(pool, T)
    for g in range(G):
        C[g, rng.integers(0, pool, per_row)] = rng.integers(1, 40, per_row)
    return C


def cap_table():
    """ the table at both limits, 1024 x 4096: four cells a row, all in the first 1024 columns -- as many wanted ids as trajectories, so
    that augmenting paths grow long while the NumPy form still ends within seconds """
    return sparse_table(5, 1024, 4096, pool=1024)


def dense_table(seed, G, T, top=3):
    """ G x T int32 counts in [0, top): ties rule """
    return np.random.default_rng(seed).integers(0, top, (G, T)).astype(np.int32)
