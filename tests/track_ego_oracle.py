""" The loop-written oracle of the tracker's ego-motion step (include/gpp.h, gpp_track_ego_f64): step 1b in plain
Python floats, one slot and one operation at a time, around the frame steps of tests/track_oracle.py (greedy) and
tests/track_optimal_oracle.py (optimal), which are imported and not edited.  It shares no code with utils/track.py.  Also the scenes
both test files use (tests/test_track_ego_cpu.py, tests/test_track_ego_gpu.py).

How a step that lies BETWEEN two statements of an imported function is placed around it: the oracle's step begins with the prediction
x += v.  Here the prediction (1a) and the ego step (1b) are done first; then the slot's velocity is put aside and replaced by 0.0, so
that the imported step's own prediction adds 0.0 and leaves the compensated position as it is, and its update leaves 0.0 + b r = b r in
the velocity.  Behind the step the velocity of a slot that still holds the same track is v' + (b r) -- the same two rounded operations
as the rule's v' + b r -- or v' itself where the slot was not matched.  Adding 0.0 can turn a -0.0 into +0.0 and nothing else: the
comparisons against this oracle are numeric (==), not bytes. """
import math

import numpy as np

import track_optimal_oracle as P
import track_oracle as O
from track_oracle import T, options, padding, row

FIELDS = 16                                   # GPP_TRACK_EGO_FIELDS: R row-major (9), t (3), dyaw (1), three zeros
QUARTER = math.pi / 2.0                       # the double every form adds for a quarter turn


# ---------------------------------------------------------------------------------------------------- the oracle
def step(st, rows, opt, ego, values=None, matrices=None):
    """ one frame with its ego record (a sequence of 16 floats): st is changed in place -> (rows_out, ids, hits) """
    e = [float(v) for v in ego]
    assert len(e) == FIELDS and all(math.isfinite(v) for v in e) and e[13:] == [0.0, 0.0, 0.0]
    box = st['box']
    aside = {}
    for t in range(T):
        if st['id1'][t] == 0:
            continue
        x = box[0][t] + box[7][t]                                                 # 1a
        y = box[1][t] + box[8][t]
        z = box[2][t] + box[9][t]
        vx, vy, vz = box[7][t], box[8][t], box[9][t]
        box[0][t] = ((e[0] * x + e[1] * y) + e[2] * z) + e[9]                     # 1b
        box[1][t] = ((e[3] * x + e[4] * y) + e[5] * z) + e[10]
        box[2][t] = ((e[6] * x + e[7] * y) + e[8] * z) + e[11]
        aside[t] = (st['id1'][t], (e[0] * vx + e[1] * vy) + e[2] * vz, (e[3] * vx + e[4] * vy) + e[5] * vz,
                    (e[6] * vx + e[7] * vy) + e[8] * vz)
        box[3][t] = O.wrap(box[3][t] + e[12])
        box[7][t] = box[8][t] = box[9][t] = 0.0
    if opt.get('assign') == 'optimal':
        out = P.step(st, rows, opt, values, matrices)
    else:
        out = O.step(st, rows, opt, values)
    for t, (id1, vx, vy, vz) in aside.items():
        if st['id1'][t] != id1:                                                   # died (a birth of this frame may hold the slot now)
            continue
        matched = st['misses'][t] == 0
        for k, v in ((7, vx), (8, vy), (9, vz)):
            box[k][t] = v + box[k][t] if matched else v
    return out


def track(frames, opt, ego, st=None, values=None, matrices=None):
    """ frames (N, D, 36), ego (N, 16) -> (rows_out, ids, hits, state); st is not changed.  values: a list that receives one list per
    frame, as tests/track_optimal_oracle.track fills it """
    st = O.empty() if st is None else {k: ([list(x) for x in v] if k == 'box' else list(v) if isinstance(v, list) else v) for k, v in st.items()}
    frames = np.asarray(frames, np.float32)
    assert len(ego) == len(frames)
    res = []
    for f, rec in zip(frames, ego):
        per_frame = None
        if values is not None:
            per_frame = []
            values.append(per_frame)
        res.append(step(st, f, opt, rec, per_frame, matrices))
    shape = frames.shape[:2]
    return (np.array([r[0] for r in res], np.float32).reshape(frames.shape), np.array([r[1] for r in res], np.int32).reshape(shape),
            np.array([r[2] for r in res], np.int32).reshape(shape), st)


# ---------------------------------------------------------------------------------------------------- records
def record(R, t, dyaw):
    return [float(v) for line in R for v in line] + [float(v) for v in t] + [float(dyaw), 0.0, 0.0, 0.0]


IDENTITY = record([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [0, 0, 0], 0.0)
# the signed permutations about Y: R of a turn by dyaw about the camera's Y axis is [[c, 0, s], [0, 1, 0], [-s, 0, c]]
LEFT = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]     # dyaw = +pi / 2
RIGHT = [[0, 0, -1], [0, 1, 0], [1, 0, 0]]    # dyaw = -pi / 2
BACK = [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]    # dyaw = pi
EYE = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
TURNS = [record(LEFT, [0.5, 0.125, -0.25], QUARTER), record(EYE, [-1.5, 0.0, 0.75], 0.0), record(RIGHT, [2.0, -0.125, 1.0], -QUARTER),
         record(BACK, [0.25, 0.0, -3.0], math.pi), record(LEFT, [0.0, 0.0, 0.0], QUARTER)]
SHIFTS = [record(EYE, [0.5, 0.125, -0.25], 0.0), record(EYE, [-1.5, 0.0, 0.75], 0.0), record(EYE, [2.0, -0.125, 1.0], 0.0)]


def cycle(records, n):
    return [records[f % len(records)] for f in range(n)]


def carry(frames, ego):
    """ a scene of a standing camera seen from the camera the records move: frame f's rows go through the records 0 .. f, one after the
    other, with the rule's own operations.  With 0 / +-1 in R and dyadic t and positions every position stays exact; r_y takes the sum of
    the dyaw, wrapped, and is rounded to float32 with the row """
    out = np.array(frames, np.float32)
    for f in range(len(out)):
        for d in range(out.shape[1]):
            r = out[f, d]
            if not r[O.ORIENT] >= 0.0:
                continue
            x, y, z, ry = float(r[O.X_]), float(r[O.Y_]), float(r[O.Z_]), float(r[O.RY_])
            for e in ego[:f + 1]:
                x, y, z = (((e[0] * x + e[1] * y) + e[2] * z) + e[9], ((e[3] * x + e[4] * y) + e[5] * z) + e[10],
                           ((e[6] * x + e[7] * y) + e[8] * z) + e[11])
                ry = O.wrap(ry + e[12])
            r[O.X_], r[O.Y_], r[O.Z_], r[O.RY_], r[20] = x, y, z, ry, y
    return out


def exact_cases():
    """ [(name, frames, ego, options)], both assignments: r_y = 0 scenes of tests/track_oracle.py carried through records whose R holds
    0 and +-1 only and whose t is dyadic, so positions, velocities and q are exact and equal candidates are equal in every form.
    Under 'dist' the records are quarter and half turns (TURNS).  Under 'bev' / '3d' the cases WITHOUT a tie go through the same turns;
    the two tie cases go through translations (SHIFTS: R = I, the trivial signed permutation): a float32 row cannot hold pi / 2, so
    behind a quarter turn the rows' rectangles are turned by 4e-8 rad against the slot's, the clipping of two mirrored rows is no longer
    the same arithmetic, and two overlaps that are equal on paper need not be equal bit for bit -- a tie there would pin cos / sin's
    last bit and not the rule """
    out = []
    for metric in ('bev', '3d', 'dist'):
        scenes = [('crossing', O.crossing(), options(metric), TURNS), ('crossing_smooth', O.crossing(), options(metric, smooth=True), TURNS),
                  ('gap_max_age', O.gap(2), options(metric), TURNS), ('gap_max_age_plus_1', O.gap(3), options(metric), TURNS),
                  ('tie_rows', O.tie_rows(), options(metric), TURNS if metric == 'dist' else SHIFTS),
                  ('tie_slots', O.tie_slots(), options(metric), TURNS if metric == 'dist' else SHIFTS)]
        for name, frames, opt, records in scenes:
            ego = cycle(records, len(frames))
            for assign in ('greedy', 'optimal'):
                o = P.optimal(opt) if assign == 'optimal' else opt
                out.append(('{}_{}_{}'.format(name, metric, assign), carry(frames, ego), np.array(ego), o))
    return out


# ---------------------------------------------------------------------------------------------------- the driving scenes
def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s, 0.0], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, 0.0], [0.0, 0.0, 0.0, 1.0]])


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0, 0.0], [0.0, c, -s, 0.0], [0.0, s, c, 0.0], [0.0, 0.0, 0.0, 1.0]])


def drive_by(seed, speed=1.5, yaw=0.04, pitch=0.0, movers=0, frames=12, cars=8, D=16, noise=0.02):
    """ `cars` cars on both kerbs (x = +-4 m, every 4 m from 10 m on) seen from a camera that drives `speed` metres per frame along its Z
    and turns `yaw` (and `pitch`) rad per frame; the first `movers` cars move +-0.4 m per frame along the world's Z, the others are
    parked; `noise` metres of Gaussian noise per coordinate; the rows of a frame in random order
    -> (frames (N, D, 36), ego (N, 16) -- row f: camera f from camera f - 1, frame 0 the identity --, per frame the car of every row) """
    rng = np.random.default_rng(seed)
    world = [np.array([-4.0 if k % 2 else 4.0, 1.65, 10.0 + 4.0 * k, 1.0]) for k in range(cars)]
    vel = [np.array([0.0, 0.0, (0.4 if k % 2 else -0.4) if k < movers else 0.0, 0.0]) for k in range(cars)]
    ry = rng.uniform(-0.2, 0.2, cars)
    dims = rng.uniform([3.4, 1.5, 1.4], [4.8, 1.9, 1.8], (cars, 3))
    advance = rot_y(yaw).dot(rot_x(pitch))
    advance[2, 3] = speed
    pose, before = np.eye(4), np.eye(4)                                           # world from camera f, and from camera f - 1
    out, ego, gts = [], [], []
    for f in range(frames):
        E = np.linalg.inv(pose).dot(before)                                       # camera f from camera f - 1
        dyaw = math.atan2(E[0, 2] - E[2, 0], E[0, 0] + E[2, 2])
        ego.append(record(E[:3, :3], E[:3, 3], dyaw))
        ry = ry + dyaw
        to_camera = np.linalg.inv(pose)
        frame, gt, order = padding(D), np.full(D, -1, np.int64), rng.permutation(D)
        for k in range(cars):
            p = to_camera.dot(world[k] + f * vel[k])[:3] + rng.normal(0.0, noise, 3)
            frame[order[k]], gt[order[k]] = row(0.9, p[0], p[2], dims[k][0], dims[k][1], ry[k], dims[k][2], p[1], 0), k
        out.append(frame)
        gts.append(gt)
        before, pose = pose, pose.dot(advance)
    return np.stack(out), np.array(ego), gts


CARS = 8
# seeds chosen on the CPU (as track_oracle.DRIVE_SEED was): the margins of tests/test_track_ego_cpu.py hold for every option below
CURVE_SEED, PITCH_SEED, STRAIGHT_SEED, MOVERS_SEED = 0, 0, 0, 0
FOR = (('dist', 1.0), ('dist', 2.0), ('bev', 0.25), ('3d', 0.25))                # the options the scenes are tracked with


def curve():
    return drive_by(CURVE_SEED)


def pitching():
    return drive_by(PITCH_SEED, pitch=0.01)


def straight():
    return drive_by(STRAIGHT_SEED, speed=2.5, yaw=0.0)


def with_movers():
    return drive_by(MOVERS_SEED, movers=2)


def margin_cases():
    """ [(name, frames, ego, options)], both assignments: general R -- tests/test_track_ego_cpu.py asserts the margins that keep the last
    bit of cos / sin out of every decision """
    out = []
    for name, (frames, ego, _) in (('curve', curve()), ('pitching', pitching())):
        for metric, thr in FOR[1:]:
            for assign in ('greedy', 'optimal'):
                for smooth in (False, True):
                    opt = options(metric, thr, smooth=smooth)
                    opt = P.optimal(opt) if assign == 'optimal' else opt
                    out.append(('{}_{}_{}{}'.format(name, metric, assign, '_smooth' if smooth else ''), frames, ego, opt))
    return out
