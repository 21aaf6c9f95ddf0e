""" A loop-written oracle of HOTA in Python integers over dicts, a float64 restatement of the metric's definition,
and the cases the HOTA tests share.  Nothing here is imported from utils/hota_eval.py.  The preprocessing -- which labels count, which rows
are kept -- and the overlaps are tests/mot_oracle.py's (section 4.29), which tests/test_mot_eval_cpu.py pins on its own. """
import numpy as np

import mot_oracle as O
from keras_retinanet_3D.utils import kitti_eval

S = 1 << 20
LEVELS = 19
NAMES = ('tp', 'fn', 'fp', 'sq', 'ass', 'assre', 'asspr')
# the definition pin's scenes: (seed, kwargs) of mot_oracle.scene
SCENES = [(31, dict(frames=40, cars=12, quantum=4)), (31, dict(frames=40, cars=12, quantum=16)), (41, dict(frames=17, cars=9, quantum=16)),
          (42, dict(frames=5, cars=20)), (7, dict(frames=12, cars=30, quantum=4)), (9, dict(frames=6, cars=70, quantum=16)),
          (11, dict(frames=30, cars=8, quantum=2, swap=0.3))]


# ---------------------------------------------------------------------------------------------------- what both restatements start from
def prepared(labels, tracks, metric='image', **limits):
    """ per sequence, per frame: {'A', 'D', 'labels': [(a, track_id)] counting, ascending, 'rows': [(d, tracker id)] kept, ascending,
    'o': {(a, d): overlap as a float}} """
    limits = dict(O.LIMITS, **limits)
    out = []
    for (lab, tids), (rows, ids) in zip(labels, tracks):
        frames = []
        for f in range(max(len(lab), len(rows))):
            g = np.asarray(lab[f], np.float64).reshape(-1, 16) if f < len(lab) else np.zeros((0, 16))
            t = [int(x) for x in np.asarray(tids[f]).reshape(-1)] if f < len(lab) else []
            r = np.asarray(rows[f], np.float32).reshape(-1, 36) if f < len(rows) else np.zeros((0, 36), np.float32)
            i = [int(x) for x in np.asarray(ids[f]).reshape(-1)] if f < len(rows) else []
            _, lout, rout, _, _ = O.frame([list(map(float, x)) for x in g], r, i, metric, limits)
            counting = [(a, t[a]) for a in range(len(g)) if lout[a] in (1, 2)]
            kept = [(d, i[d]) for d in range(len(r)) if rout[d] in (1, 3)]
            planes = kitti_eval.image_overlaps(r, g) if metric != 'image' and len(g) and len(r) else None
            o = {}
            for a, _ in counting:
                for d, _ in kept:
                    o[a, d] = O.image_overlap(r[d], g[a])[0] if metric == 'image' else float(planes[1 if metric == 'bev' else 2, d, a])
            frames.append({'A': len(g), 'D': len(r), 'labels': counting, 'rows': kept, 'o': o})
        out.append(frames)
    return out


# ---------------------------------------------------------------------------------------------------- the rules, in loops and integers
def similarity(o):
    if not o > 0.0:
        return 0
    return int(np.floor(min(o * S, float(S))))


def evaluate(labels, tracks, metric='image', **limits):
    """ -> per sequence {'P', 'A', 'hist': {(track_id, tracker id): ...}, 'gc', 'tc': {id: n}, 'frames': [{'match': [A], 'counts': [40],
    'cost': matrix}], 'ints': {name: [19]}} """
    out = []
    for frames in prepared(labels, tracks, metric, **limits):
        P, gc, tc = {}, {}, {}
        for fr in frames:
            q = {k: similarity(v) for k, v in fr['o'].items()}
            fr['q'] = q
            for a, g in fr['labels']:
                gc[g] = gc.get(g, 0) + 1
            for d, t in fr['rows']:
                tc[t] = tc.get(t, 0) + 1
            for a, g in fr['labels']:
                rs = sum(q[a, d] for d, _ in fr['rows'])
                for d, t in fr['rows']:
                    cs = sum(q[a2, d] for a2, _ in fr['labels'])
                    P.setdefault((g, t), 0)
                    if q[a, d] > 0:
                        P[g, t] += (q[a, d] * S) // (rs + cs - q[a, d])
        align = {k: (v * S) // ((gc[k[0]] + tc[k[1]]) * S - v) if v > 0 else 0 for k, v in P.items()}
        hist, per_frame = {}, []
        tp, sq, n_g, n_t = [0] * (LEVELS + 1), [0] * (LEVELS + 1), 0, 0
        for fr in frames:
            q, G, T = fr['q'], len(fr['labels']), len(fr['rows'])
            n = max(G, T)
            cost = [[S] * n for _ in range(n)]
            for i, (a, g) in enumerate(fr['labels']):
                for j, (d, t) in enumerate(fr['rows']):
                    cost[i][j] = S - ((align[g, t] * q[a, d]) >> 20)
            col = O.assign(cost)
            match, counts = [-1] * fr['A'], [0] * 40
            for i, (a, g) in enumerate(fr['labels']):
                if col[i] >= T:
                    continue
                d, t = fr['rows'][col[i]]
                jm = min(LEVELS, (20 * q[a, d] + 19) >> 20)
                if jm < 1:
                    continue
                match[a] = d
                hist.setdefault((g, t), [0] * (LEVELS + 1))[jm] += 1
                for j in range(1, jm + 1):
                    tp[j] += 1
                    sq[j] += q[a, d]
                    counts[j - 1] += 1
                    counts[LEVELS + j - 1] += q[a, d]
            counts[38], counts[39] = G, T
            n_g, n_t = n_g + G, n_t + T
            per_frame.append({'match': match, 'counts': counts, 'cost': cost})
        ints = {name: [0] * LEVELS for name in NAMES}
        for j in range(1, LEVELS + 1):
            ints['tp'][j - 1], ints['sq'][j - 1] = tp[j], sq[j]
            ints['fn'][j - 1], ints['fp'][j - 1] = n_g - tp[j], n_t - tp[j]
            for (g, t), h in hist.items():
                mc = sum(h[j:])
                if mc > 0:
                    ints['ass'][j - 1] += (mc * mc * S) // (gc[g] + tc[t] - mc)
                    ints['assre'][j - 1] += (mc * mc * S) // gc[g]
                    ints['asspr'][j - 1] += (mc * mc * S) // tc[t]
        out.append({'P': P, 'A': align, 'hist': hist, 'gc': gc, 'tc': tc, 'frames': per_frame, 'ints': ints})
    return out


# ---------------------------------------------------------------------------------------------------- the definition, in float64
def float_hota(labels, tracks, metric='image', eps=np.finfo(np.float64).eps, **limits):
    """ HOTA as its definition states it (Luiten et al., IJCV 2021), in float64 on the same preprocessing: the similarity s, the potential
    as float sums of s / (row sum + column sum - s), the alignment A = P / (gc + tc - P), scipy's optimal assignment on -A s per frame,
    a pair counts at threshold j iff s >= j / 20 - eps, the association sums as floats.
    -> per sequence {'pairs': [per frame {(a, d)} at the lowest threshold], 'tp': [19], and per threshold the ratios} """
    from scipy.optimize import linear_sum_assignment
    out = []
    for frames in prepared(labels, tracks, metric, **limits):
        gts = sorted({g for fr in frames for _, g in fr['labels']})
        trs = sorted({t for fr in frames for _, t in fr['rows']})
        gi, ti = {g: k for k, g in enumerate(gts)}, {t: k for k, t in enumerate(trs)}
        P, gc, tc = np.zeros((len(gts), len(trs))), np.zeros(len(gts)), np.zeros(len(trs))
        sims = []
        for fr in frames:
            s = np.zeros((len(fr['labels']), len(fr['rows'])))
            for i, (a, _) in enumerate(fr['labels']):
                for j, (d, _) in enumerate(fr['rows']):
                    s[i, j] = min(max(fr['o'][a, d], 0.0), 1.0) if fr['o'][a, d] == fr['o'][a, d] else 0.0
            sims.append(s)
            g = [gi[x] for _, x in fr['labels']]
            t = [ti[x] for _, x in fr['rows']]
            den = s.sum(axis=1, keepdims=True) + s.sum(axis=0, keepdims=True) - s
            share = np.zeros_like(s)
            share[den > eps] = s[den > eps] / den[den > eps]
            if s.size:
                P[np.ix_(g, t)] += share
            gc[g] += 1
            tc[t] += 1
        align = P / np.maximum(gc[:, None] + tc[None, :] - P, eps)
        mc = np.zeros((LEVELS,) + P.shape)
        tp, loc, pairs = np.zeros(LEVELS), np.zeros(LEVELS), []
        n_g = n_t = 0
        for fr, s in zip(frames, sims):
            g = [gi[x] for _, x in fr['labels']]
            t = [ti[x] for _, x in fr['rows']]
            n_g, n_t = n_g + len(g), n_t + len(t)
            found = set()
            if s.size:
                ri, ci = linear_sum_assignment(-(align[np.ix_(g, t)] * s))
                for i, j in zip(ri, ci):
                    for k in range(LEVELS):
                        if s[i, j] >= (k + 1) / 20.0 - eps:
                            mc[k, g[i], t[j]] += 1
                            tp[k] += 1
                            loc[k] += s[i, j]
                            found.add((fr['labels'][i][0], fr['rows'][j][0]))
            pairs.append(found)
        res = {'pairs': pairs, 'tp': [int(v) for v in tp]}
        for name in ('deta', 'detre', 'detpr', 'assa', 'assre', 'asspr', 'loca', 'hota'):
            res[name] = []
        for k in range(LEVELS):
            fn, fp = n_g - tp[k], n_t - tp[k]
            on = mc[k] > 0
            m = mc[k][on]
            ass = (m * m / (gc[:, None] + tc[None, :] - mc[k])[on]).sum()
            assre = (m * m / np.broadcast_to(gc[:, None], P.shape)[on]).sum()
            asspr = (m * m / np.broadcast_to(tc[None, :], P.shape)[on]).sum()
            div = lambda x, y, empty=0.0: x / y if y > 0 else empty  # noqa: E731
            res['deta'].append(div(tp[k], tp[k] + fn + fp))
            res['detre'].append(div(tp[k], tp[k] + fn))
            res['detpr'].append(div(tp[k], tp[k] + fp))
            res['assa'].append(div(ass, tp[k]))
            res['assre'].append(div(assre, tp[k]))
            res['asspr'].append(div(asspr, tp[k]))
            res['loca'].append(div(loc[k], tp[k], 1.0))
            res['hota'].append(np.sqrt(res['deta'][-1] * res['assa'][-1]))
        out.append(res)
    return out


# ---------------------------------------------------------------------------------------------------- the cases
def split_case():
    """ one car, 6 frames, followed by id 7 for three frames and by id 9 for three, rows = labels """
    labs = [np.stack([O.label(0, (100.0 + 8 * f, 100.0, 200.0 + 8 * f, 180.0))]) for f in range(6)]
    return [(labs, [np.array([3])] * 6)], [([O.rows_of(g) for g in labs], [np.array([7])] * 3 + [np.array([9])] * 3)]


def tie_case():
    """ alignment breaks a tie: one car followed by id 7 for three frames; in the fourth frame two identical rows, id 9 first, then id 7 """
    labs = [np.stack([O.label(0, (100.0 + 8 * f, 100.0, 200.0 + 8 * f, 180.0))]) for f in range(4)]
    rows = [O.rows_of(g) for g in labs[:3]] + [O.rows_of([labs[3][0], labs[3][0]])]
    return [(labs, [np.array([3])] * 4)], [(rows, [np.array([7])] * 3 + [np.array([9, 7])])]


def dense_sequence():
    """ four dense frames that share label and tracker ids: pair-table rows and columns beyond 64, cells that many frames add to """
    labs, tids, rows, ids = [], [], [], []
    for k, (G, T) in enumerate([(65, 66), (128, 128), (64, 64), (66, 65)]):
        (g, t), (r, i) = O.dense(900 + k, G, T)
        labs, tids, rows, ids = labs + g, tids + t, rows + r, ids + i
    return [(labs, tids)], [(rows, ids)]
