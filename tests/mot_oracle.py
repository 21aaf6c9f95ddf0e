""" A loop-written oracle of the tracking score in Python integers, and the cases the tests share.  Nothing here is
vectorised and nothing is imported from utils/mot_eval.py: the image overlap is written out, the assignment is the textbook 1-based form of
the shortest-augmenting-path method with a virtual column 0.  The BEV and 3-D overlaps are taken from utils/kitti_eval.image_overlaps, which
tests/test_kitti_eval_cpu.py pins on its own. """
import numpy as np

from keras_retinanet_3D.utils import kitti_eval

SCALE = 1 << 20
BIG = 1 << 28
LIMITS = {'min_overlap': 0.5, 'max_occlusion': 2.0, 'max_truncation': 0.0, 'min_height': 25.0}
COUNT_NAMES = ('tp', 'fp', 'fn', 'n_gt', 'sum_k', 'cost', 'ids', 'frag', 'mt', 'pt', 'ml', 'trajectories', 'frames')


# ---------------------------------------------------------------------------------------------------- the rules, in loops
def image_overlap(row, label):
    """ (IoU, intersection over the row's area) of a pose row's box (columns 26-29) and a label's (columns 4-7) """
    dx1, dy1, dx2, dy2 = (float(row[c]) for c in (26, 27, 28, 29))
    gx1, gy1, gx2, gy2 = (float(label[c]) for c in (4, 5, 6, 7))
    w = min(dx2, gx2) - max(dx1, gx1)
    h = min(dy2, gy2) - max(dy1, gy1)
    if w <= 0.0 or h <= 0.0:
        return 0.0, 0.0
    inter = w * h
    area_d, area_g = (dx2 - dx1) * (dy2 - dy1), (gx2 - gx1) * (gy2 - gy1)
    return inter / (area_d + area_g - inter), inter / area_d


def status(label, limits):
    """ 'count', 'ignore', 'dontcare' or None """
    kind, trunc, occ = int(label[0]), float(label[1]), float(label[2])
    if kind == 0:
        hard = occ > limits['max_occlusion'] or trunc > limits['max_truncation'] or abs(float(label[7]) - float(label[5])) < limits['min_height']
        return 'ignore' if hard else 'count'
    return {1: 'ignore', 2: 'dontcare'}.get(kind)


def assign(cost):
    """ cost: n lists of n Python ints -> the column of every row """
    n = len(cost)
    INF = 1 << 62
    u, v, p, way = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    for i in range(1, n + 1):
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
    col = [0] * n
    for j in range(1, n + 1):
        col[p[j] - 1] = j - 1
    return col


def frame(labels, rows, ids, metric, limits):
    """ one frame -> (match [A], label_outcome [A], row_outcome [D], counts [8], cost matrix) """
    A, D = len(labels), len(rows)
    stat = [status(g, limits) for g in labels]
    live = [float(rows[d][14]) >= 0.0 and int(ids[d]) >= 0 for d in range(D)]
    gl = [a for a in range(A) if stat[a] in ('count', 'ignore')]
    rl = [d for d in range(D) if live[d]]
    planes = kitti_eval.image_overlaps(np.asarray(rows, np.float32).reshape(-1, 36), np.asarray(labels, np.float64).reshape(-1, 16)) if metric != 'image' else None
    n = max(len(gl), len(rl))
    cost = [[BIG] * n for _ in range(n)]
    for g, a in enumerate(gl):
        for t, d in enumerate(rl):
            o = image_overlap(rows[d], labels[a])[0] if metric == 'image' else float(planes[1 if metric == 'bev' else 2, d, a])
            if o >= limits['min_overlap']:
                cost[g][t] = SCALE - int(np.floor(min(o * SCALE, float(SCALE))))
    col = assign(cost)
    match, lout, rout = [-1] * A, [0] * A, [0] * D
    tp = fp = fn = n_gt = sum_k = 0
    paired_rows = set()
    for g, a in enumerate(gl):
        t = col[g]
        paired = t < len(rl) and cost[g][t] < BIG
        if stat[a] == 'count':
            n_gt += 1
        if paired:
            match[a] = rl[t]
            paired_rows.add(rl[t])
            if stat[a] == 'count':
                lout[a], rout[rl[t]] = 1, 1
                tp += 1
                sum_k += SCALE - cost[g][t]
            else:
                lout[a], rout[rl[t]] = 3, 2
        elif stat[a] == 'count':
            lout[a] = 2
            fn += 1
        else:
            lout[a] = 4
    for d in rl:
        if d in paired_rows:
            continue
        if abs(float(rows[d][29]) - float(rows[d][27])) < limits['min_height']:
            rout[d] = 4
        elif any(stat[a] == 'dontcare' and image_overlap(rows[d], labels[a])[1] > 0.5 for a in range(A)):
            rout[d] = 5
        else:
            rout[d] = 3
            fp += 1
    total = sum(cost[g][col[g]] for g in range(n))
    return match, lout, rout, [tp, fp, fn, n_gt, sum_k, total, len(gl), len(rl)], cost


def evaluate(labels, tracks, metric='image', **limits):
    """ labels: per sequence (labels_per_frame, track_ids_per_frame); tracks: per sequence (rows_per_frame, ids_per_frame) ->
    {'sequences': [dict of the 13 integers], 'tables': [{track_id: [counting, matched, switches, fragmentations]}],
     'frames': [[(match, label_outcome, row_outcome, counts)]], 'costs': [[matrix]]} """
    limits = dict(LIMITS, **limits)
    out = {'sequences': [], 'tables': [], 'frames': [], 'costs': []}
    for (lab, tids), (rows, ids) in zip(labels, tracks):
        N = max(len(lab), len(rows))
        sums = [0] * 6
        state, per_frame, costs = {}, [], []
        for f in range(N):
            g = [list(map(float, x)) for x in np.asarray(lab[f], np.float64).reshape(-1, 16)] if f < len(lab) else []
            t = [int(x) for x in np.asarray(tids[f]).reshape(-1)] if f < len(lab) else []
            r = np.asarray(rows[f], np.float32).reshape(-1, 36) if f < len(rows) else np.zeros((0, 36), np.float32)
            i = [int(x) for x in np.asarray(ids[f]).reshape(-1)] if f < len(rows) else []
            match, lout, rout, counts, cost = frame(g, r, i, metric, limits)
            per_frame.append((match, lout, rout, counts))
            costs.append(cost)
            for k in range(6):
                sums[k] += counts[k]
            for a in range(len(g)):
                if lout[a] not in (1, 2):
                    continue
                st = state.setdefault(t[a], {'n': 0, 'm': 0, 'ids': 0, 'frag': 0, 'last': None, 'gap': False})
                st['n'] += 1
                if lout[a] == 2:
                    st['gap'] = True
                    continue
                st['m'] += 1
                if st['last'] is not None:
                    st['ids'] += st['last'] != i[match[a]]
                    st['frag'] += st['gap']
                st['last'], st['gap'] = i[match[a]], False
        mt = sum(1 for s in state.values() if 5 * s['m'] >= 4 * s['n'])
        ml = sum(1 for s in state.values() if 5 * s['m'] < s['n'])
        counts = sums + [sum(s['ids'] for s in state.values()), sum(s['frag'] for s in state.values()), mt, len(state) - mt - ml, ml, len(state), N]
        out['sequences'].append(dict(zip(COUNT_NAMES, counts)))
        out['tables'].append({k: [s['n'], s['m'], s['ids'], s['frag']] for k, s in state.items()})
        out['frames'].append(per_frame)
        out['costs'].append(costs)
    return out


def greedy_pairs(cost):
    """ best-overlap-first greedy on a cost matrix: the number of pairs below BIG it finds (what every other matcher of the project does) """
    cells = sorted((c, g, t) for g, line in enumerate(cost) for t, c in enumerate(line) if c < BIG)
    rows_taken, cols_taken = set(), set()
    for c, g, t in cells:
        if g not in rows_taken and t not in cols_taken:
            rows_taken.add(g)
            cols_taken.add(t)
    return len(rows_taken)


# ---------------------------------------------------------------------------------------------------- building blocks
def label(kind, box, trunc=0.0, occ=0.0, ry=0.0):
    """ a (16,) label row: kind 0 Car, 1 Van, 2 DontCare, 3 Pedestrian; the cuboid follows the box, so that every metric sees the scene """
    x1, y1, x2, y2 = box
    return np.array([kind, trunc, occ, 0.0, x1, y1, x2, y2, 1.5, (x2 - x1) / 32.0, (y2 - y1) / 16.0, x1 / 16.0, 1.65, 20.0 + y1 / 8.0, ry, 0.0])


def row_of(lab, score=1.0):
    """ the pose row that says exactly what a label says """
    line = np.array(lab, np.float64).reshape(1, 16).copy()
    line[0, 0], line[0, 15] = 0.0, score
    return kitti_eval.rows_from_results(line)[0]


def rows_of(labs):
    return np.stack([row_of(g) for g in labs]) if len(labs) else np.zeros((0, 36), np.float32)


def two_cars(frames=5):
    boxes = lambda f: [(100.0 + 8 * f, 100.0, 200.0 + 8 * f, 180.0), (300.0 - 8 * f, 120.0, 420.0 - 8 * f, 200.0)]  # noqa: E731
    labs = [np.stack([label(0, b) for b in boxes(f)]) for f in range(frames)]
    return labs, [np.array([3, 5])] * frames


def named_cases():
    """ {name: (labels, tracks, expect of the sequence 0 / of 'all', options)} -- the issue's cases """
    cases = {}
    labs, tids = two_cars()
    rows = [rows_of(g) for g in labs]
    cases['perfect'] = ([(labs, tids)], [(rows, [np.array([7, 9])] * 5)],
                        dict(tp=10, fp=0, fn=0, ids=0, frag=0, mt=2, pt=0, ml=0, n_gt=10, mota=1.0, motp=1.0), {})
    cases['swap'] = ([(labs, tids)], [(rows, [np.array([7, 9])] * 3 + [np.array([9, 7])] * 2)],
                     dict(tp=10, fp=0, fn=0, ids=2, frag=0, mt=2, mota=0.8, motp=1.0), {})
    gap_rows = [r if f != 2 else r[1:] for f, r in enumerate(rows)]
    gap_ids = [np.array([7, 9]) if f != 2 else np.array([9]) for f in range(5)]
    cases['gap'] = ([(labs, tids)], [(gap_rows, gap_ids)], dict(tp=9, fp=0, fn=1, ids=0, frag=1, mt=2, pt=0, ml=0, mota=0.9), {})
    # optimal beats greedy: label 0 overlaps row 1 by 56 / 72 and row 0 by 48 / 80; label 1 overlaps row 1 by 48 / 80 and row 0 by 24 / 104
    g = np.stack([label(0, (100.0, 100.0, 164.0, 164.0)), label(0, (124.0, 100.0, 188.0, 164.0))])
    r = rows_of([label(0, (84.0, 100.0, 148.0, 164.0)), label(0, (108.0, 100.0, 172.0, 164.0))])
    cases['optimal_beats_greedy'] = ([([g], [np.array([0, 1])])], [([r], [np.array([4, 6])])], dict(tp=2, fp=0, fn=0, mota=1.0), {})
    # ignored: a matched Van, a row inside a DontCare, a row of height 20, a Car of occlusion 3 -- and a Pedestrian, not in play
    g = np.stack([label(1, (100.0, 100.0, 200.0, 180.0)), label(2, (300.0, 50.0, 500.0, 250.0)), label(0, (600.0, 100.0, 700.0, 180.0), occ=3.0),
                  label(3, (800.0, 100.0, 840.0, 200.0))])
    r = rows_of([label(0, (100.0, 100.0, 200.0, 180.0)), label(0, (320.0, 100.0, 400.0, 180.0)), label(0, (900.0, 100.0, 960.0, 120.0))])
    cases['ignored'] = ([([g], [np.array([1, -1, 2, 3])])], [([r], [np.array([0, 1, 2])])],
                        dict(tp=0, fp=0, fn=0, n_gt=0, trajectories=0, mota=None, motp=None), {})
    # threshold: 64 / 128 is exactly 0.5 and matches; 64 / (128 + 2^-12) is one quantum of 2^-20 below and does not
    g = [np.stack([label(0, (0.0, 100.0, 96.0, 164.0))])] * 2
    r = [rows_of([label(0, (32.0, 100.0, 128.0, 164.0))]), rows_of([label(0, (32.0, 100.0, 128.0 + 2.0 ** -12, 164.0))])]
    cases['threshold'] = ([(g, [np.array([0])] * 2)], [(r, [np.array([0])] * 2)], dict(tp=1, fp=1, fn=1, sum_k=1 << 19, ids=0), {})
    # ties: two labels and two rows, all four overlaps equal
    g = np.stack([label(0, (100.0, 100.0, 200.0, 180.0))] * 2)
    cases['ties'] = ([([g], [np.array([0, 1])])], [([rows_of(g)], [np.array([5, 6])])], dict(tp=2, fp=0, fn=0), {})
    # empty: a frame without labels, one without rows, one with neither; and a sequence of no frames
    g = [np.zeros((0, 16)), np.stack([label(0, (100.0, 100.0, 200.0, 180.0))]), np.zeros((0, 16))]
    r = [rows_of([label(0, (100.0, 100.0, 200.0, 180.0))]), np.zeros((0, 36), np.float32), np.zeros((0, 36), np.float32)]
    cases['empty'] = ([(g, [np.zeros(0, int), np.array([0]), np.zeros(0, int)]), ([], [])],
                      [(r, [np.array([0]), np.zeros(0, int), np.zeros(0, int)]), ([], [])],
                      dict(tp=0, fp=1, fn=1, n_gt=1, ml=1, frames=3, mota=-1.0, motp=None), {})
    return cases


# ---------------------------------------------------------------------------------------------------- seeded scenes
def scene(seed, frames=8, cars=6, quantum=8.0, drop=0.15, clutter=2, swap=0.1):
    """ one sequence: cars (some Vans, some occluded, some low), DontCare regions and Pedestrians on a grid of `quantum` pixels, rows that
    follow the labels with jitter of a few quanta, missing rows, spurious rows and ids that sometimes change hands -> (labels, tracks).
    A coarse quantum makes many overlaps equal. """
    rng = np.random.default_rng(seed)
    x = rng.integers(2, 60, cars) * 16.0
    y = rng.integers(4, 12, cars) * 16.0
    w = rng.integers(2, 6, cars) * 32.0
    h = np.where(rng.random(cars) < 0.15, 16.0, rng.integers(2, 5, cars) * 16.0)
    kind = rng.choice([0, 0, 0, 0, 1], cars)
    occ = rng.choice([0.0, 1.0, 2.0, 3.0], cars, p=[0.5, 0.2, 0.15, 0.15])
    step = rng.integers(-2, 3, cars) * quantum
    tracker = np.arange(cars) + 10
    labs, tids, rows, ids = [], [], [], []
    for f in range(frames):
        if rng.random() < swap and cars >= 2:
            a, b = rng.choice(cars, 2, replace=False)
            tracker[a], tracker[b] = tracker[b], tracker[a]
        seen = rng.random(cars) < 0.9                                       # a label is not in every frame
        g, t, r, i = [], [], [], []
        for c in np.flatnonzero(seen):
            bx = x[c] + step[c] * f
            g.append(label(kind[c], (bx, y[c], bx + w[c], y[c] + h[c]), occ=occ[c], ry=0.0))
            t.append(c)
            if rng.random() >= drop:
                jx, jy = rng.integers(-2, 3) * quantum, rng.integers(-1, 2) * quantum
                r.append(label(0, (bx + jx, y[c] + jy, bx + jx + w[c], y[c] + jy + h[c])))
                i.append(tracker[c])
        g.append(label(2, (0.0, 300.0, 400.0, 370.0)))
        t.append(-1)
        g.append(label(3, (500.0, 300.0, 530.0, 370.0)))
        t.append(100)
        for c in range(clutter):
            bx, by = rng.integers(0, 60) * 16.0, rng.choice([96.0, 310.0])
            r.append(label(0, (bx, by, bx + 64.0, by + rng.choice([16.0, 48.0]))))
            i.append(200 + c)
        order = rng.permutation(len(r))
        labs.append(np.stack(g))
        tids.append(np.array(t))
        rows.append(rows_of([r[k] for k in order]))
        ids.append(np.array([i[k] for k in order], np.int32).reshape(-1))
    return (labs, tids), (rows, ids)


def dense(seed, G, T, shift=16.0, far=False):
    """ one frame of G Car labels in a line, each overlapping its neighbours admissibly (boxes 64 wide, `shift` apart: 48 / 80), and T rows
    on the same line, 0, 8 or 16 further -- many equal overlaps, rows that two labels want alike, long augmenting paths.  far: the rows lie where nothing overlaps """
    rng = np.random.default_rng(seed)
    g = np.stack([label(0, (shift * k, 100.0, shift * k + 64.0, 164.0)) for k in range(G)]) if G else np.zeros((0, 16))
    at = rng.permutation(max(G, T))[:T] * shift + rng.integers(0, 3, T) * 8.0       # (8: halfway between two labels, 56 / 72 with both)
    r = rows_of([label(0, (x, 400.0 if far else 100.0, x + 64.0, 464.0 if far else 164.0)) for x in at])
    return ([g], [np.arange(G)]), ([r], [np.arange(T, dtype=np.int32) + 50])
