""" The loop-written oracle of the tracker (include/gpp.h, gpp_track_f64): plain Python floats, one slot, one row
and one candidate at a time, written from the specification.  It shares no code with utils/track.py or utils/kitti_eval.py; the rectangle
clipping is the other oracle's (tests/cuboid_nms_oracle.py).  Also the scenes both test files use (tests/test_track_cpu.py,
tests/test_track_gpu.py). """
import math

import numpy as np

from cuboid_nms_oracle import COLS, area, clip, corners, nan_row, padding, row

T = 128
SCORE, ORIENT = 12, 14
X_, Y_, Z_, RY_, H_, W_, L_ = 19, 31, 21, 32, 30, 17, 18
FIELD_COLS = (X_, Y_, Z_, RY_, H_, W_, L_)            # the row's column of the state's fields 0..6; 7..9 are vx vy vz
PI = math.pi
TWO_PI = 2.0 * math.pi


# ---------------------------------------------------------------------------------------------------- the oracle
def empty():
    return {'id1': [0] * T, 'hits': [0] * T, 'misses': [0] * T, 'score': [0.0] * T, 'box': [[0.0] * T for _ in range(10)],
            'next_id': 0, 'frames': 0, 'dropped': 0}


def wrap(a):
    a = a - TWO_PI * math.floor(a / TWO_PI)
    if a < 0.0:
        a += TWO_PI
    if a >= TWO_PI:
        a -= TWO_PI
    if a >= PI:
        a -= TWO_PI
    return a


def pair_value(box, t, r, metric):
    """ the overlap (or q) of slot t's predicted cuboid and the row r (a list of floats) """
    x, y, z, ry, h, w, l = [box[k][t] for k in range(7)]
    if metric == 'dist':
        dx, dz = r[X_] - x, r[Z_] - z
        return dx * dx + dz * dz
    poly = corners(l, w, x, z, ry)
    g = corners(r[L_], r[W_], r[X_], r[Z_], r[RY_])
    for e in range(4):
        poly = clip(poly, g[e], g[(e + 1) % 4])
    inter = area(poly)
    area_t, area_r = l * w, r[L_] * r[W_]
    if metric == 'bev':
        den = area_t + area_r - inter
        return inter / den if den != 0.0 else float('nan')
    hh = max(0.0, min(y, r[Y_]) - max(y - h, r[Y_] - r[H_]))
    iv = inter * hh
    den = area_t * h + area_r * r[H_] - iv
    return iv / den if den != 0.0 else float('nan')


def step(st, rows, opt, values=None):
    """ one frame: st is changed in place -> (rows_out (D, 36) float32, ids [D], hits [D]).  values: a list that receives
    (value, slot, row) of every pair of an occupied slot and a live, non-blind row (the margins) """
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
    cands = []                                                                    # 3
    for t in occupied:
        for d in valid:
            v = pair_value(box, t, R[d], metric)
            if values is not None:
                values.append((v, t, d))
            if metric == 'dist':
                if v < thr * thr:
                    cands.append((v, t, d))
            elif v > thr:
                cands.append((-v, t, d))
    cands.sort()                                                                  # 4: best first, then slot, then row
    slot_row, row_slot = {}, {}
    for _, t, d in cands:
        if t not in slot_row and d not in row_slot:
            slot_row[t], row_slot[d] = d, t
    for t, d in slot_row.items():                                                 # 5
        for k in range(3):
            pred = box[k][t]
            r = R[d][FIELD_COLS[k]] - pred
            box[k][t] = pred + a * r
            box[7 + k][t] = box[7 + k][t] + b * r
        for k in (4, 5, 6):
            box[k][t] = box[k][t] + c * (R[d][FIELD_COLS[k]] - box[k][t])
        delta = wrap(R[d][RY_] - box[3][t])
        if delta >= PI / 2.0:
            delta -= PI
        if delta < -(PI / 2.0):
            delta += PI
        box[3][t] = wrap(box[3][t] + a * delta)
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
            out[d][25] = np.float32(wrap(box[3][t] - math.atan2(box[0][t], box[2][t])))
    return out, ids, hits


def track(frames, opt, st=None, values=None):
    """ frames: (N, D, 36) -> (rows_out (N, D, 36), ids (N, D) int32, hits (N, D) int32, state); st is not changed """
    st = empty() if st is None else {k: ([list(x) for x in v] if k == 'box' else list(v) if isinstance(v, list) else v) for k, v in st.items()}
    frames = np.asarray(frames, np.float32)
    res = [step(st, f, opt, values) for f in frames]
    shape = frames.shape[:2]
    return (np.array([r[0] for r in res], np.float32).reshape(frames.shape), np.array([r[1] for r in res], np.int32).reshape(shape),
            np.array([r[2] for r in res], np.int32).reshape(shape), st)


def same_state(st, record):
    """ the oracle's state against one STATE_DTYPE record of utils/track.py: every field, == """
    return (np.array_equal(np.array(st['id1'], np.int32), record['id1']) and np.array_equal(np.array(st['hits'], np.int32), record['hits'])
            and np.array_equal(np.array(st['misses'], np.int32), record['misses'])
            and np.array_equal(np.array(st['score'], np.float32), record['score'])
            and np.array_equal(np.array(st['box'], np.float64), record['box'])
            and (st['next_id'], st['frames'], st['dropped']) == (int(record['next_id']), int(record['frames']), int(record['dropped'])))


def margins(values, opt):
    """ (the smallest distance of a pair's value from the threshold -- q from threshold^2 --, the smallest distance between the values of
    two candidates of one frame); values: per frame the list that `step` fills """
    thr = opt['threshold'] * opt['threshold'] if opt['metric'] == 'dist' else opt['threshold']
    to_thr, apart = math.inf, math.inf
    for frame in values:
        vs = [v for v, _, _ in frame if not math.isnan(v)]
        to_thr = min([to_thr] + [abs(v - thr) for v in vs])
        cand = sorted(v for v in vs if (v < thr if opt['metric'] == 'dist' else v > thr))
        apart = min([apart] + [q - p for p, q in zip(cand, cand[1:])])
    return to_thr, apart


def frame_values(frames, opt, st=None):
    """ per frame the values of `step`, for margins """
    st = empty() if st is None else st
    out = []
    for f in np.asarray(frames, np.float32):
        out.append([])
        step(st, f, opt, out[-1])
    return out


# ---------------------------------------------------------------------------------------------------- the scenes
GAINS = (0.5, 0.25, 0.25)                     # dyadic: with r_y = 0 and dyadic positions and sizes every step is exact
# thresholds no value of an exact case can meet: overlaps of dyadic boxes are ratios of small dyadic numbers, q a multiple of 2^-12
IOU_THR, DIST_THR = 0.2718, 2.3


def options(metric, threshold=None, max_age=2, gains=GAINS, birth_score=0.0, smooth=False):
    threshold = (DIST_THR if metric == 'dist' else IOU_THR) if threshold is None else threshold
    return {'metric': metric, 'threshold': threshold, 'max_age': max_age, 'gains': gains, 'birth_score': birth_score, 'smooth': smooth}


def frames_of(lists, D):
    """ per frame a list of rows -> (N, D, 36) with padding behind """
    return np.stack([np.concatenate([np.stack(rs) if rs else np.zeros((0, COLS), np.float32), padding(D - len(rs))]) for rs in lists])


def crossing():
    """ case 1: two cars whose paths cross, one lane apart: x = -4 + f and 4 - f at z = 20 and 21 """
    return frames_of([[row(0.9, -4.0 + f, 20.0), row(0.8, 4.0 - f, 21.0)] for f in range(9)], 3)


def gap(missing):
    """ case 2: a car seen three times, missing `missing` frames, seen again """
    car = [row(0.9, 0.5, 20.0)]
    return frames_of([car] * 3 + [[]] * missing + [car] * 2, 2)


def tie_rows():
    """ case 3a: one slot, two rows equally good: the smaller row wins """
    return frames_of([[row(0.9, 0.0, 20.0)], [row(0.8, 1.0, 20.0), row(0.7, -1.0, 20.0)]], 2)


def tie_slots():
    """ case 3b: two slots equally good for one row: the smaller slot wins """
    return frames_of([[row(0.9, 1.0, 20.0), row(0.8, -1.0, 20.0)], [row(0.7, 0.0, 20.0)]], 2)


def full_house():
    """ case 4: 128 cars on a grid fill every slot; in frame 1 the last one is gone and one more stands elsewhere """
    grid = [row(0.5 + k / 256.0, 8.0 * (k % 16), 16.0 + 8.0 * (k // 16)) for k in range(128)]
    return np.stack([np.stack(grid), np.stack(grid[:127] + [row(0.75, -16.0, 16.0)])])


def odd_rows():
    """ case 5: blind rows, padding between the rows, a frame without rows """
    car, other = row(0.9, 0.0, 20.0), row(0.8, 8.0, 24.0)
    return np.stack([np.stack([padding()[0], car, nan_row(0.95, 0.25, 20.0), other]),
                     np.stack([nan_row(0.9, 0.0, 20.0), padding()[0], other, car]),
                     padding(4),
                     np.stack([car, other, padding()[0], nan_row(0.5, 8.0, 24.0)])])


def turned():
    """ case 6: a detection whose r_y is off by pi, and a pair of r_y either side of +-pi """
    flip = wrap(0.3 + PI)
    return frames_of([[row(0.9, 0.0, 20.0, ry=0.3), row(0.8, 10.0, 30.0, ry=3.13)],
                      [row(0.9, 0.1, 20.1, ry=flip), row(0.8, 10.1, 30.1, ry=-3.13)],
                      [row(0.9, 0.2, 20.2, ry=0.32), row(0.8, 10.2, 30.2, ry=3.12)]], 2)


def drive(seed, frames=12, cars=6, D=16, noise=0.05, max_age=2, lane=6.0, with_gt=False):
    """ cases 7, 8 and the CPU suite's long scene: `cars` cars in lanes `lane` metres apart, constant velocity along z, `noise` metres of
    Gaussian noise per coordinate, every car missing in at most max_age consecutive frames, the rows of a frame in random order """
    rng = np.random.default_rng(seed)
    x0 = [lane * (k - cars / 2.0) for k in range(cars)]
    z0, vz = rng.uniform(20.0, 40.0, cars), rng.uniform(-0.5, 0.5, cars)
    ry, dims = rng.uniform(-PI, PI, cars), rng.uniform([3.4, 1.5, 1.4], [4.8, 1.9, 1.8], (cars, 3))
    run = [0] * cars
    out, gts = [], []
    for f in range(frames):
        rs, gt = [], []
        for k in range(cars):
            if run[k] < max_age and rng.uniform() < 0.3:
                run[k] += 1
                continue
            run[k] = 0
            rs.append(row(rng.uniform(0.3, 1.0), x0[k] + rng.normal(0.0, noise), z0[k] + vz[k] * f + rng.normal(0.0, noise), dims[k][0],
                          dims[k][1], ry[k] + rng.normal(0.0, 0.02), dims[k][2], 1.65 + rng.normal(0.0, noise), int(rng.integers(0, 4))))
            gt.append(k)
        order = rng.permutation(D)
        frame, g = padding(D), np.full(D, -1, np.int64)
        for k, r in enumerate(rs):
            frame[order[k]], g[order[k]] = r, gt[k]
        out.append(frame)
        gts.append(g)
    return (np.stack(out), gts) if with_gt else np.stack(out)


DRIVE_SEED = 11                               # chosen on the CPU: the margins of test_track_cpu.py hold for all three metrics


def exact_cases():
    """ [(name, frames, options)]: r_y = 0 and dyadic numbers -- equal candidates are equal in every form """
    out = []
    for metric in ('bev', '3d', 'dist'):
        out += [('crossing', crossing(), options(metric)), ('crossing_smooth', crossing(), options(metric, smooth=True)),
                ('gap_max_age', gap(2), options(metric)), ('gap_max_age_plus_1', gap(3), options(metric)),
                ('tie_rows', tie_rows(), options(metric)), ('tie_slots', tie_slots(), options(metric)),
                ('odd_rows', odd_rows(), options(metric)), ('birth_score', crossing(), options(metric, birth_score=0.85))]
    out += [('full_house', full_house(), options('dist')), ('full_house', full_house(), options('bev'))]
    return [('{}_{}'.format(n, o['metric']), f, o) for n, f, o in out]


def margin_cases():
    """ [(name, frames, options)]: general r_y -- the margins of test_track_cpu.py keep cos / sin's last bit out of every decision """
    out = []
    for metric in ('bev', '3d', 'dist'):
        out += [('turned', turned(), options(metric, smooth=True)), ('drive', drive(DRIVE_SEED), options(metric)),
                ('drive_smooth', drive(DRIVE_SEED), options(metric, smooth=True, gains=(0.6, 0.3, 0.1)))]
    return [('{}_{}'.format(n, o['metric']), f, o) for n, f, o in out]
