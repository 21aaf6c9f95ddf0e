""" The loop-written oracle of the tracker's Kalman filter (include/gpp.h, gpp_track_kf_f64): the whole frame step in
plain Python floats, one slot, one row, one pair and one operation at a time, transcribed from the specification's parenthesised
expressions.  It shares no code with utils/track.py; the pair values of 'bev' / '3d' / 'dist', the wrap and the scene builders are
tests/track_oracle.py's, the optimal form's cell and augmenting-path loop tests/track_optimal_oracle.py's, the ego records
tests/track_ego_oracle.py's -- all imported, none edited.  Also the scenes both test files use (tests/test_track_kf_cpu.py,
tests/test_track_kf_gpu.py). """
import math

import numpy as np

import track_ego_oracle as E
import track_optimal_oracle as P
import track_oracle as O
from track_oracle import COLS, FIELD_COLS, ORIENT, PI, RY_, SCORE, T, X_, Z_, frames_of, padding, row

AXX, AXZ, AZZ, BXX, BXZ, BZX, BZZ, CXX, CXZ, CZZ = range(10)

# the issue's demonstration values; dyadic gains as everywhere
NOISE = {'radial': (0.1, 0.05), 'tangential': (0.1, 0.005), 'process': (0.01, 0.01), 'birth_speed': 2.0}
GATE = 3.0


# ---------------------------------------------------------------------------------------------------- the oracle
def empty_cov():
    return [[0.0] * T for _ in range(10)]


def row_noise(x, z, noise):
    (r0, r1), (t0, t1) = noise['radial'], noise['tangential']
    rho = math.sqrt((x * x) + (z * z))
    if rho == 0.0:
        ux, uz = 0.0, 1.0
    else:
        ux, uz = x / rho, z / rho
    sr = r0 + (r1 * rho)
    st = t0 + (t1 * rho)
    vr, vt = sr * sr, st * st
    dv = vr - vt
    return vt + (dv * (ux * ux)), dv * (ux * uz), vt + (dv * (uz * uz))


def turn(g, xx, xz, zx, zz):
    g00, g01, g10, g11 = g
    mxx = (g00 * xx) + (g01 * zx)
    mxz = (g00 * xz) + (g01 * zz)
    mzx = (g10 * xx) + (g11 * zx)
    mzz = (g10 * xz) + (g11 * zz)
    return (mxx * g00) + (mxz * g01), (mxx * g10) + (mxz * g11), (mzx * g00) + (mzz * g01), (mzx * g10) + (mzz * g11)


def born(cov, t, R, speed):
    cov[AXX][t], cov[AXZ][t], cov[AZZ][t] = R
    for k in (BXX, BXZ, BZX, BZZ, CXZ):
        cov[k][t] = 0.0
    cov[CXX][t] = cov[CZZ][t] = speed * speed


def divide(a, b):
    """ IEEE division for the one denominator that can be zero (a caller's covariance) """
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def step(st, cov, rows, opt, ego=None, values=None, branches=None, matrices=None):
    """ one frame: st and cov are changed in place -> (rows_out (D, 36) float32, ids [D], hits [D]).  values receives (value, slot, row)
    of every pair of an occupied slot and a live, non-blind row; branches receives 'kalman' or 'fallback' per matched pair; matrices
    (optimal) receives (cost, slots, rows, pairs) of the frame, as tests/track_optimal_oracle.step gives them """
    metric, thr, max_age, birth, smooth = opt['metric'], opt['threshold'], opt['max_age'], opt['birth_score'], opt['smooth']
    a, b, c = opt['gains']
    noise = opt['noise']
    q_pos, q_vel = noise['process']
    speed = noise['birth_speed']
    box = st['box']
    rows = np.asarray(rows, np.float32).reshape(-1, COLS)
    D = len(rows)
    R = [[float(rows[d][k]) for k in range(COLS)] for d in range(D)]
    occupied = [t for t in range(T) if st['id1'][t] != 0]
    for t in occupied:                                                            # 1
        for k in range(3):
            box[k][t] = box[k][t] + box[7 + k][t]
        p = [cov[k][t] for k in range(10)]
        cov[AXX][t] = ((p[AXX] + (p[BXX] + p[BXX])) + p[CXX]) + q_pos
        cov[AXZ][t] = (p[AXZ] + (p[BXZ] + p[BZX])) + p[CXZ]
        cov[AZZ][t] = ((p[AZZ] + (p[BZZ] + p[BZZ])) + p[CZZ]) + q_pos
        cov[BXX][t] = p[BXX] + p[CXX]
        cov[BXZ][t] = p[BXZ] + p[CXZ]
        cov[BZX][t] = p[BZX] + p[CXZ]
        cov[BZZ][t] = p[BZZ] + p[CZZ]
        cov[CXX][t] = p[CXX] + q_vel
        cov[CZZ][t] = p[CZZ] + q_vel
        if ego is not None:                                                       # 1b
            e = [float(v) for v in ego]
            x, y, z = box[0][t], box[1][t], box[2][t]
            vx, vy, vz = box[7][t], box[8][t], box[9][t]
            box[0][t] = ((e[0] * x + e[1] * y) + e[2] * z) + e[9]
            box[1][t] = ((e[3] * x + e[4] * y) + e[5] * z) + e[10]
            box[2][t] = ((e[6] * x + e[7] * y) + e[8] * z) + e[11]
            box[7][t] = (e[0] * vx + e[1] * vy) + e[2] * vz
            box[8][t] = (e[3] * vx + e[4] * vy) + e[5] * vz
            box[9][t] = (e[6] * vx + e[7] * vy) + e[8] * vz
            box[3][t] = O.wrap(box[3][t] + e[12])
            g = (e[0], e[2], e[6], e[8])
            p = [cov[k][t] for k in range(10)]
            cov[AXX][t], cov[AXZ][t], _, cov[AZZ][t] = turn(g, p[AXX], p[AXZ], p[AXZ], p[AZZ])
            cov[BXX][t], cov[BXZ][t], cov[BZX][t], cov[BZZ][t] = turn(g, p[BXX], p[BXZ], p[BZX], p[BZZ])
            cov[CXX][t], cov[CXZ][t], _, cov[CZZ][t] = turn(g, p[CXX], p[CXZ], p[CXZ], p[CZZ])
    live = [d for d in range(D) if R[d][ORIENT] >= 0.0]                           # 2
    valid = [d for d in live if not any(math.isnan(R[d][k]) for k in FIELD_COLS)]
    noise_of = {d: row_noise(R[d][X_], R[d][Z_], noise) for d in valid}

    def innovation(t, d):
        sxx, sxz, szz = cov[AXX][t] + noise_of[d][0], cov[AXZ][t] + noise_of[d][1], cov[AZZ][t] + noise_of[d][2]
        return sxx, sxz, szz, (sxx * szz) - (sxz * sxz)

    cands = {}                                                                    # 3: (slot, row) -> the value
    for t in occupied:
        for d in valid:
            if metric == 'maha':
                sxx, sxz, szz, det = innovation(t, d)
                dx, dz = R[d][X_] - box[0][t], R[d][Z_] - box[2][t]
                v = divide((((szz * dx) * dx) - ((2.0 * (sxz * dx)) * dz)) + ((sxx * dz) * dz), det)
                ok = det > 0.0 and v < thr * thr
            else:
                v = O.pair_value(box, t, R[d], metric)
                ok = (v < thr * thr) if metric == 'dist' else (v > thr)
            if values is not None:
                values.append((v, t, d))
            if ok:
                cands[(t, d)] = v
    slot_row, row_slot = {}, {}                                                   # 4
    if opt.get('assign') == 'optimal':
        n = max(len(occupied), len(valid))
        cost = [[P.S] * n for _ in range(n)]
        for (t, d), v in cands.items():
            cost[occupied.index(t)][valid.index(d)] = P.cell(v, 'dist' if metric == 'maha' else metric, thr)
        p = P.assign(cost)
        for j, d in enumerate(valid):
            i = p[j]
            if i < len(occupied) and cost[i][j] < P.S:
                slot_row[occupied[i]], row_slot[d] = d, occupied[i]
        if matrices is not None:
            matrices.append((cost, occupied, valid, sorted(slot_row.items())))
    else:
        keyed = sorted(((v if metric in ('dist', 'maha') else -v), t, d) for (t, d), v in cands.items())
        for _, t, d in keyed:
            if t not in slot_row and d not in row_slot:
                slot_row[t], row_slot[d] = d, t
    for t, d in slot_row.items():                                                 # 5
        sxx, sxz, szz, det = innovation(t, d)
        kalman = det > 0.0
        if branches is not None:
            branches.append('kalman' if kalman else 'fallback')
        if kalman:
            p = [cov[k][t] for k in range(10)]
            px, pz = box[0][t], box[2][t]
            dx, dz = R[d][X_] - px, R[d][Z_] - pz
            ixx, ixz, izz = szz / det, -(sxz / det), sxx / det
            kxx, kxz = (p[AXX] * ixx) + (p[AXZ] * ixz), (p[AXX] * ixz) + (p[AXZ] * izz)
            kzx, kzz = (p[AXZ] * ixx) + (p[AZZ] * ixz), (p[AXZ] * ixz) + (p[AZZ] * izz)
            lxx, lxz = (p[BXX] * ixx) + (p[BZX] * ixz), (p[BXX] * ixz) + (p[BZX] * izz)
            lzx, lzz = (p[BXZ] * ixx) + (p[BZZ] * ixz), (p[BXZ] * ixz) + (p[BZZ] * izz)
            box[0][t] = px + ((kxx * dx) + (kxz * dz))
            box[2][t] = pz + ((kzx * dx) + (kzz * dz))
            box[7][t] = box[7][t] + ((lxx * dx) + (lxz * dz))
            box[9][t] = box[9][t] + ((lzx * dx) + (lzz * dz))
            cov[AXX][t] = p[AXX] - ((kxx * p[AXX]) + (kxz * p[AXZ]))
            cov[AXZ][t] = p[AXZ] - ((kxx * p[AXZ]) + (kxz * p[AZZ]))
            cov[AZZ][t] = p[AZZ] - ((kzx * p[AXZ]) + (kzz * p[AZZ]))
            cov[BXX][t] = p[BXX] - ((kxx * p[BXX]) + (kxz * p[BZX]))
            cov[BXZ][t] = p[BXZ] - ((kxx * p[BXZ]) + (kxz * p[BZZ]))
            cov[BZX][t] = p[BZX] - ((kzx * p[BXX]) + (kzz * p[BZX]))
            cov[BZZ][t] = p[BZZ] - ((kzx * p[BXZ]) + (kzz * p[BZZ]))
            cov[CXX][t] = p[CXX] - ((lxx * p[BXX]) + (lxz * p[BZX]))
            cov[CXZ][t] = p[CXZ] - ((lxx * p[BXZ]) + (lxz * p[BZZ]))
            cov[CZZ][t] = p[CZZ] - ((lzx * p[BXZ]) + (lzz * p[BZZ]))
        else:
            born(cov, t, noise_of[d], speed)
        for k in range(3):
            if kalman and k != 1:
                continue
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
                cov[k][t] = 0.0
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
        born(cov, t, noise_of[d], speed)
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


def copy_state(st):
    return {k: ([list(x) for x in v] if k == 'box' else list(v) if isinstance(v, list) else v) for k, v in st.items()}


def track(frames, opt, ego=None, st=None, cov=None, values=None, branches=None, matrices=None):
    """ frames (N, D, 36), ego None or (N, 16) -> (rows_out, ids, hits, state, cov); st and cov are not changed.  values receives one
    list per frame """
    st = O.empty() if st is None else copy_state(st)
    cov = empty_cov() if cov is None else [[float(v) for v in line] for line in cov]
    frames = np.asarray(frames, np.float32)
    res = []
    for f, rows in enumerate(frames):
        per_frame = None
        if values is not None:
            per_frame = []
            values.append(per_frame)
        res.append(step(st, cov, rows, opt, None if ego is None else ego[f], per_frame, branches, matrices))
    shape = frames.shape[:2]
    return (np.array([r[0] for r in res], np.float32).reshape(frames.shape), np.array([r[1] for r in res], np.int32).reshape(shape),
            np.array([r[2] for r in res], np.int32).reshape(shape), st, cov)


def same_cov(cov, array):
    """ the oracle's covariance against a (10, 128) float64 array: every word, == """
    return np.array_equal(np.array(cov, np.float64), np.asarray(array))


# ---------------------------------------------------------------------------------------------------- options and scenes
def options(metric, threshold=None, assign='greedy', noise=NOISE, **more):
    """ an option with the filter; 'maha' gates at GATE standard deviations unless told otherwise """
    if metric == 'maha':
        opt = O.options('dist', GATE if threshold is None else threshold, **more)
        opt['metric'] = 'maha'
    else:
        opt = O.options(metric, threshold, **more)
    opt.update(filter='kalman', noise=noise)
    return P.optimal(opt) if assign == 'optimal' else opt


def plain(opt):
    """ the same option without the filter (for a metric the fixed-gain tracker has) """
    return {k: v for k, v in opt.items() if k not in ('filter', 'noise')}


def demo():
    """ the issue's scene, 12 frames from a still camera: F at (2, 60) measured at z = 60 +- 3 (+ on even frames), P at (-2, 10) exactly
    in frames 0 - 5, Q at (1.5, 12.5) from frame 6 on -> (frames (12, 2, 36), per frame the car of every row: 0 F, 1 P, 2 Q) """
    lists, gts = [], []
    for f in range(12):
        far = row(0.9, 2.0, 60.0 + (3.0 if f % 2 == 0 else -3.0))
        near = row(0.8, -2.0, 10.0) if f < 6 else row(0.8, 1.5, 12.5)
        lists.append([far, near])
        gts.append(np.array([0, 1 if f < 6 else 2]))
    return frames_of(lists, 2), gts


DEMO_DIST = (2.0, 3.0, 4.0, 4.25, 4.5, 5.0, 6.0, 8.0)


def mover(frames=6):
    """ a car born moving: 1 m per frame along z from (0.5, 20), exact rows """
    return frames_of([[row(0.9, 0.5, 20.0 + f)] for f in range(frames)], 2)


def steady(frames=200):
    """ one car seen in every frame at 0.25 m per frame, with a deterministic +-0.125 m wobble: 200 matched updates """
    return frames_of([[row(0.9, 3.0 + (0.125 if f % 3 == 0 else -0.0625), 15.0 + 0.25 * f + (0.125 if f % 2 else -0.125))] for f in range(frames)], 1)


def general_record():
    """ one general rotation: yaw 0.04 and pitch 0.01, a translation """
    pose = E.rot_y(0.04).dot(E.rot_x(0.01))
    R, t = pose[:3, :3], [0.125, -0.03125, -1.5]
    return E.record(R, t, math.atan2(R[0][2] - R[2][0], R[0][0] + R[2][2]))


def ego_kinds(n):
    """ {name: (n, 16) records}: identity records, quarter turns, one general rotation among identities """
    return {'identity': np.array(E.cycle([E.IDENTITY], n)), 'turns': np.array(E.cycle(E.TURNS, n)),
            'general': np.array([general_record() if f == 1 else E.IDENTITY for f in range(n)])}


DRIVE = O.drive(O.DRIVE_SEED, frames=12, cars=6, D=8)
THRESHOLDS = {'maha': GATE, 'dist': 2.3, 'bev': 0.2718, '3d': 0.2718}


def cases():
    """ [(name, frames, ego or None, options)]: all four metrics x both assignments x (no records, identity records, quarter turns, one
    general rotation), D <= 8, <= 12 frames.  Without records and under the identity the scene is track_oracle.drive (general r_y);
    under the turns it is track_oracle.crossing carried through the records (exact positions); the general rotation moves the drive's
    carried cuboids once, by a few centimetres at these ranges """
    out = []
    crossing = O.crossing()
    for metric in ('maha', 'dist', 'bev', '3d'):
        for assign in ('greedy', 'optimal'):
            opt = options(metric, THRESHOLDS[metric], assign, smooth=(assign == 'optimal'))
            out.append(('drive_{}_{}'.format(metric, assign), DRIVE, None, opt))
            for kind, ego in ego_kinds(len(DRIVE)).items():
                if kind == 'turns':
                    recs = ego[:len(crossing)]
                    out.append(('crossing_turns_{}_{}'.format(metric, assign), E.carry(crossing, [list(r) for r in recs]), recs, opt))
                else:
                    out.append(('drive_{}_{}_{}'.format(kind, metric, assign), DRIVE, ego, opt))
    return out


def margins(values, opt):
    """ tests/track_oracle.margins with 'maha' read as 'dist' (m against threshold^2) """
    return O.margins(values, dict(opt, metric='dist') if opt['metric'] == 'maha' else opt)
