""" The loop-written oracle of the tracker's optimal assignment (include/gpp.h, gpp_track_optimal_f64): plain
Python integers and floats, one slot, one row, one cell and one column at a time, written from the specification -- the frame step of
section 4.28 with its step 4 replaced, and the augmenting-path loop of the header's paragraph "assignment".  It shares no code with
utils/track.py or utils/mot_eval.py; the pair values, the wrap and the scene builders are tests/track_oracle.py's.  Also the scenes both
test files use (tests/test_track_optimal_cpu.py, tests/test_track_optimal_gpu.py). """
import math

import numpy as np

import track_oracle as O
from track_oracle import COLS, FIELD_COLS, ORIENT, PI, RY_, SCORE, T, frames_of, options, padding, row

S = 1 << 20                                   # GPP_MOT_SCALE_BITS: the cell of a pair that is no candidate, and of padding


# ---------------------------------------------------------------------------------------------------- the oracle
def cell(value, metric, thr):
    """ the cell of a CANDIDATE whose value is q ('dist') or the overlap """
    if metric == 'dist':
        t2 = thr * thr
        r = value / t2
        x = r * 1048576.0
        return min(int(math.floor(x)), S - 1)
    k = int(math.floor(min(value * 1048576.0, 1048576.0)))
    return min(S - k, S - 1)


def assign(cost):
    """ the header's paragraph: rows in order, one shortest augmenting path each -> p, the row every column holds """
    n = len(cost)
    u, v, p = [0] * n, [0] * n, [-1] * n
    for i in range(n):
        minv, way, used = [None] * n, [-1] * n, [False] * n           # None: infinity
        i0, came_from = i, -1
        while True:
            for j in range(n):
                if used[j]:
                    continue
                cur = cost[i0][j] - u[i0] - v[j]
                if minv[j] is None or cur < minv[j]:
                    minv[j], way[j] = cur, came_from
            delta, j1 = None, -1
            for j in range(n):                                       # the FIRST column that has the smallest minv
                if not used[j] and (delta is None or minv[j] < delta):
                    delta, j1 = minv[j], j
            u[i] += delta
            for j in range(n):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            used[j1] = True
            came_from = j1
            if p[j1] < 0:
                break
            i0 = p[j1]
        j = j1                                                       # the rows are handed back along way, j1 first
        while way[j] >= 0:
            p[j] = p[way[j]]
            j = way[j]
        p[j] = i
    return p


def step(st, rows, opt, values=None, matrices=None):
    """ one frame: st is changed in place -> (rows_out (D, 36) float32, ids [D], hits [D]).  values: as tests/track_oracle.step;
    matrices: a list that receives (cost, slots, rows, pairs) of the frame """
    metric, thr, max_age, birth, smooth = opt['metric'], opt['threshold'], opt['max_age'], opt['birth_score'], opt['smooth']
    a, b, c = opt['gains']
    box = st['box']
    rows = np.asarray(rows, np.float32).reshape(-1, COLS)
    D = len(rows)
    R = [[float(rows[d][k]) for k in range(COLS)] for d in range(D)]
    occupied = [t for t in range(T) if st['id1'][t] != 0]
    for t in occupied:                                                            # 1
        for k in range(3):
            box[k][t] = box[k][t] + box[7 + k][t]
    live = [d for d in range(D) if R[d][ORIENT] >= 0.0]                           # 2
    valid = [d for d in live if not any(math.isnan(R[d][k]) for k in FIELD_COLS)]
    n = max(len(occupied), len(valid))                                            # 3 and the matrix
    cost = [[S] * n for _ in range(n)]
    for i, t in enumerate(occupied):
        for j, d in enumerate(valid):
            v = O.pair_value(box, t, R[d], metric)
            if values is not None:
                values.append((v, t, d))
            if (v < thr * thr) if metric == 'dist' else (v > thr):
                cost[i][j] = cell(v, metric, thr)
    p = assign(cost)                                                              # 4
    slot_row, row_slot = {}, {}
    for j, d in enumerate(valid):
        i = p[j]
        if i < len(occupied) and cost[i][j] < S:
            slot_row[occupied[i]], row_slot[d] = d, occupied[i]
    if matrices is not None:
        matrices.append((cost, occupied, valid, sorted(slot_row.items())))
    for t, d in slot_row.items():                                                 # 5
        for k in range(3):
            pred = box[k][t]
            r = R[d][FIELD_COLS[k]] - pred
            box[k][t] = pred + a * r
            box[7 + k][t] = box[7 + k][t] + b * r
        for k in (4, 5, 6):
            box[k][t] = box[k][t] + c * (R[d][FIELD_COLS[k]] - box[k][t])
        delta = O.wrap(R[d][RY_] - box[3][t])
        if delta >= PI / 2.0:
            delta -= PI
        if delta < -(PI / 2.0):
            delta += PI
        box[3][t] = O.wrap(box[3][t] + a * delta)
        st['hits'][t] += 1
        st['misses'][t] = 0
        st['score'][t] = R[d][SCORE]
    for t in occupied:                                                            # 6
        if t in slot_row:
            continue
        st['misses'][t] += 1
        if st['misses'][t] > max_age:
            st['id1'][t] = st['hits'][t] = st['misses'][t] = 0
            st['score'][t] = 0.0
            for k in range(10):
                box[k][t] = 0.0
    for d in valid:                                                               # 7
        if d in row_slot or not R[d][SCORE] >= birth:
            continue
        free = [t for t in range(T) if st['id1'][t] == 0]
        if not free:
            st['dropped'] += 1
            continue
        t = free[0]
        st['id1'][t] = st['next_id'] + 1
        st['next_id'] += 1
        st['hits'][t], st['misses'][t], st['score'][t] = 1, 0, R[d][SCORE]
        for k in range(7):
            box[k][t] = R[d][FIELD_COLS[k]]
        for k in (7, 8, 9):
            box[k][t] = 0.0
        row_slot[d] = t
    st['frames'] += 1
    out = rows.copy()                                                             # 8
    ids, hits = [-1] * D, [0] * D
    for d, t in row_slot.items():
        ids[d], hits[d] = st['id1'][t] - 1, st['hits'][t]
        if smooth:
            for k in range(7):
                out[d][FIELD_COLS[k]] = np.float32(box[k][t])
            out[d][25] = np.float32(O.wrap(box[3][t] - math.atan2(box[0][t], box[2][t])))
    return out, ids, hits


def track(frames, opt, st=None, values=None, matrices=None):
    """ frames: (N, D, 36) -> (rows_out (N, D, 36), ids (N, D) int32, hits (N, D) int32, state); st is not changed.  values, matrices:
    lists that receive one list (values) or one tuple (matrices) per frame """
    st = O.empty() if st is None else {k: ([list(x) for x in v] if k == 'box' else list(v) if isinstance(v, list) else v) for k, v in st.items()}
    frames = np.asarray(frames, np.float32)
    res = []
    for f in frames:
        per_frame = None
        if values is not None:
            per_frame = []
            values.append(per_frame)
        res.append(step(st, f, opt, per_frame, matrices))
    shape = frames.shape[:2]
    return (np.array([r[0] for r in res], np.float32).reshape(frames.shape), np.array([r[1] for r in res], np.int32).reshape(shape),
            np.array([r[2] for r in res], np.int32).reshape(shape), st)


# ---------------------------------------------------------------------------------------------------- the scenes
def optimal(opt):
    return dict(opt, assign='optimal')


def steal():
    """ two tracks at x = 0 and 2, then rows at x = 0.875 and -1: greedy gives the nearer row to track 0, track 1 misses and a third id is
    born; the optimum pairs both.  ('dist', 2.0): the cells are [[200704, 262144], [331776, 2^20]] """
    return frames_of([[row(0.9, 0.0, 20.0), row(0.8, 2.0, 20.0)], [row(0.9, 0.875, 20.0), row(0.8, -1.0, 20.0)]], 2)


STEAL_OPTION = options('dist', threshold=2.0)


def one_slot_three_rows():
    return frames_of([[row(0.9, 0.0, 20.0)], [row(0.8, 1.0, 20.0), row(0.7, 0.5, 20.0), row(0.6, -0.75, 20.0)]], 3)


def three_slots_one_row():
    return frames_of([[row(0.9, -1.0, 20.0), row(0.8, 0.75, 20.0), row(0.7, 1.0, 20.0)], [row(0.6, 0.5, 20.0)]], 3)


def one_sided():
    """ a frame without slots and without rows (n = 0), rows but no slots, slots but no rows, then the match """
    car = [row(0.9, 0.5, 20.0)]
    return frames_of([[], car, [], car], 2)


def grid_car(k, score=None, dx=0.0):
    return row(0.5 + k / 256.0 if score is None else score, 8.0 * (k % 16) + dx, 16.0 + 8.0 * (k // 16))


def many_slots_two_rows():
    """ 65 slots against 2 rows: the matrix's rows reach index 64 (the lane's second potential), and slot 64 is matched """
    first = [grid_car(k) for k in range(65)]
    second = [grid_car(64, 0.75, 0.5), grid_car(3, 0.625, -0.25)] + [padding()[0]] * 63
    return np.stack([np.stack(first), np.stack(second)])


def two_slots_many_rows():
    """ 2 slots against 65 rows at D = 65: the matched columns are 3 and 64 (the lane's second column) """
    first = [grid_car(100), grid_car(101)] + [padding()[0]] * 63
    second = [grid_car(k) for k in range(65)]
    second[64], second[3] = grid_car(100, 0.75, 0.5), grid_car(101, 0.625, -0.25)
    return np.stack([np.stack(first), np.stack(second)])


def dense_drive(with_gt=False):
    """ ten cars in lanes 1.75 m apart with 0.4 m of noise: neighbours compete for detections """
    return O.drive(O.DRIVE_SEED, frames=30, cars=10, lane=1.75, noise=0.4, with_gt=with_gt)


def exact_cases():
    """ [(name, frames, options)]: tests/track_oracle.exact_cases() with the optimal assignment, and the smallest shapes that reach each
    branch of the new step; r_y = 0 and dyadic numbers -- the three forms are equal with ==, ties included """
    out = [(n, f, optimal(o)) for n, f, o in O.exact_cases()]
    for metric in ('bev', '3d', 'dist'):
        for name, frames in (('one_slot_three_rows', one_slot_three_rows()), ('three_slots_one_row', three_slots_one_row()),
                             ('one_sided', one_sided()), ('many_slots_two_rows', many_slots_two_rows()),
                             ('two_slots_many_rows', two_slots_many_rows())):
            out.append(('{}_{}'.format(name, metric), frames, optimal(options(metric))))
    out.append(('steal_dist', steal(), optimal(STEAL_OPTION)))
    return out


def margin_cases():
    """ [(name, frames, options)]: general r_y -- tests/test_track_optimal_cpu.py asserts the margins that keep the last bit of cos / sin
    out of every decision """
    return [(n, f, optimal(o)) for n, f, o in O.margin_cases()] + [('dense_drive_dist', dense_drive(), optimal(options('dist')))]
