"""
Tracking of cuboids across frames: the pose rows of one frame are associated greedily with the cuboids carried over from the frames
before, and every carried cuboid is a fixed-gain (alpha-beta) filter -- DESIGN.md section 4.28 is the specification, include/gpp.h
(gpp_track_f64, gpp_track_state) the contract.  With 'assign': 'optimal' the association is the optimal one-to-one assignment of the
frame instead (gpp_track_optimal_f64); everything else is the same step.  With `ego` records (DESIGN.md section 4.33,
gpp_track_ego_f64) the carried cuboids are moved into every frame's camera coordinates before they are matched: the camera of a driving car
moves, and a parked car must not.  With 'filter': 'kalman' (gpp_track_kf_f64) every carried cuboid keeps the
covariance of (x, z, vx, vz) beside the state: a row's noise grows with its range along the viewing ray, a matched pair is updated with
the Kalman gain, and the fourth metric 'maha' gates and ranks by the squared Mahalanobis distance.  An identity per car that persists from
frame to frame, and optionally a pose that does not jump by the detector's depth jitter.  There is no default threshold: it depends on
the checkpoint and the frame rate.

Two forms of one computation:
    track_rows_np        NumPy, no GPU and no library: the candidates of a frame at once (the clipping of utils/kitti_eval.py), the
                         greedy pass serial over the sorted candidates, as the rule demands ('optimal': utils/mot_eval.assign_np on the
                         frame's integer cells).
    track_rows_device    csrc/track.hip: one launch, one workgroup per sequence.

The state is one record of STATE_DTYPE, byte for byte the gpp_track_state of include/gpp.h; all zero bytes is the empty tracker.
"""
import numpy as np

from . import gpp_utils, kitti_eval, mot_eval, track_kf as KF
from .track_kf import PI, wrap              # wrap: into [-pi, pi), as csrc/pose.hip; importers of utils.track find both names here

METRICS = ('bev', '3d', 'dist')             # include/gpp.h: GPP_TRACK_BEV 0, GPP_TRACK_3D 1, GPP_TRACK_DIST 2
POSE_COLS = kitti_eval.POSE_COLS
MAX_DETECTIONS = kitti_eval.MAX_DETECTIONS  # what the device form takes per frame
MAX_TRACKS = 128                            # GPP_TRACK_MAX_TRACKS
FIELDS = ('x', 'y', 'z', 'r_y', 'h', 'w', 'l', 'vx', 'vy', 'vz')
ROW_COLS = [19, 31, 21, 32, 30, 17, 18]     # the pose row's column of the first seven fields
STATE_DTYPE = np.dtype([('id1', '<i4', (MAX_TRACKS,)), ('hits', '<i4', (MAX_TRACKS,)), ('misses', '<i4', (MAX_TRACKS,)),
                        ('score', '<f4', (MAX_TRACKS,)), ('box', '<f8', (len(FIELDS), MAX_TRACKS)),
                        ('next_id', '<i4'), ('frames', '<i4'), ('dropped', '<i4'), ('reserved', '<i4')])
# gains and max_age: chosen on synthetic constant-velocity scenes only (tests/track_oracle.py); no real sequence has been measured
DEFAULTS = {'max_age': 2, 'gains': (0.5, 0.25, 0.25), 'birth_score': 0.0, 'smooth': False}
ASSIGNS = ('greedy', 'optimal')             # gpp_track_f64, gpp_track_optimal_f64; 'greedy' is the default and is not carried in the option
SCALE = mot_eval.SCALE                      # 2^20 (GPP_MOT_SCALE_BITS): the cell of a pair that is no candidate
TRACKING_FORMAT = '%d %d ' + gpp_utils.KITTI_FORMAT
EGO_FIELDS = 16                             # GPP_TRACK_EGO_FIELDS: R row-major (9), t (3), dyaw (1), three words that are 0
KF_METRICS = METRICS + ('maha',)            # GPP_TRACK_MAHA 3: only with 'filter': 'kalman' (gpp_track_kf_f64)
FILTERS = ('fixed', 'kalman')               # 'fixed' (the gains) is the default and is not carried in the option
COV_FIELDS = ('Axx', 'Axz', 'Azz', 'Bxx', 'Bxz', 'Bzx', 'Bzz', 'Cxx', 'Cxz', 'Czz')      # gpp_track_cov: p[field][slot]
NOISE_KEYS = ('radial', 'tangential', 'process', 'birth_speed')


def metric_code(metric, kalman=False):
    if metric not in (KF_METRICS if kalman else METRICS):
        if metric == 'maha':
            raise ValueError("track: the metric 'maha' needs 'filter': 'kalman' and its 'noise'")
        raise ValueError("track: the metric must be 'bev', '3d' or 'dist', got {!r}".format(metric))
    return KF_METRICS.index(metric)


def check_noise(noise):
    """ the 'noise' of a Kalman option -> {'radial': (r0, r1), 'tangential': (t0, t1), 'process': (q_pos, q_vel), 'birth_speed': v0} of
    floats; ValueError for what gpp_track_kf_f64 refuses.  There are no defaults: nothing here has seen a real sequence """
    if not isinstance(noise, dict) or sorted(noise) != sorted(NOISE_KEYS):
        raise ValueError("track: 'noise' must be a dict with exactly {}, got {!r}".format(list(NOISE_KEYS), noise))
    out = {}
    for key in NOISE_KEYS[:3]:
        try:
            v0, v1 = [float(v) for v in noise[key]]
        except (TypeError, ValueError):
            raise ValueError('track: noise[{!r}] must be two numbers, got {!r}'.format(key, noise[key]))
        out[key] = (v0, v1)
    try:
        out['birth_speed'] = float(noise['birth_speed'])
    except (TypeError, ValueError):
        raise ValueError("track: noise['birth_speed'] must be a number, got {!r}".format(noise['birth_speed']))
    positive = (out['radial'][0], out['tangential'][0], out['birth_speed'])
    rest = (out['radial'][1], out['tangential'][1]) + out['process']
    if not all(np.isfinite(v) and v > 0.0 for v in positive):
        raise ValueError('track: radial[0], tangential[0] and birth_speed must be finite and > 0, got {!r}'.format(positive))
    if not all(np.isfinite(v) and v >= 0.0 for v in rest):
        raise ValueError('track: radial[1], tangential[1] and process must be finite and >= 0, got {!r}'.format(rest))
    return out


def check_option(option):
    """ the `track` option of load_model / RetinaNet3D: None, a pair (metric, threshold), or a dict with 'metric' and 'threshold' and
    optionally 'max_age', 'gains' (a, b, c), 'birth_score', 'smooth', 'assign' ('greedy' | 'optimal'), 'ego' (True | False: the model
    takes ego records, section 4.33), 'filter' ('fixed' | 'kalman', section 4.34) with, for 'kalman', the required 'noise' (check_noise)
    -> None or the complete dict; it carries 'assign' only when that is 'optimal', 'ego' only when that is true, 'filter' and 'noise'
    only for 'kalman'.  The metric 'maha' (threshold: standard deviations) needs the Kalman filter """
    if option is None:
        return None
    if isinstance(option, dict):
        unknown = sorted(set(option) - {'metric', 'threshold', 'assign', 'ego', 'filter', 'noise'} - set(DEFAULTS))
        if unknown or 'metric' not in option or 'threshold' not in option:
            raise ValueError("track: a dict needs 'metric' and 'threshold' and may have {}; got {!r}".format(sorted(DEFAULTS) + ['assign', 'ego', 'filter', 'noise'], option))
        opt = dict(DEFAULTS, **option)
    else:
        try:
            metric, threshold = option
        except (TypeError, ValueError):
            raise ValueError("track must be None, a pair (metric, threshold) such as ('dist', 2.0) or a dict, got {!r}".format(option))
        opt = dict(DEFAULTS, metric=metric, threshold=threshold)
    kind = opt.get('filter', 'fixed')
    if not isinstance(kind, str) or kind not in FILTERS:
        raise ValueError("track: filter must be 'fixed' or 'kalman', got {!r}".format(kind))
    if kind == 'kalman' and 'noise' not in opt:
        raise ValueError("track: 'filter': 'kalman' needs 'noise' -- there are no defaults, nothing here has seen a real sequence")
    if kind != 'kalman' and 'noise' in opt:
        raise ValueError("track: 'noise' is the Kalman filter's: it needs 'filter': 'kalman'")
    noise = check_noise(opt['noise']) if kind == 'kalman' else None
    code = metric_code(opt['metric'], kind == 'kalman')
    thr = float(opt['threshold'])
    if code >= 2 and not (np.isfinite(thr) and thr > 0.0):
        raise ValueError('track: a {} threshold must be finite and positive, got {!r}'.format(opt['metric'], thr))
    if code < 2 and not 0.0 <= thr < 1.0:
        raise ValueError('track: an overlap threshold must lie inside [0, 1), got {!r}'.format(thr))
    try:
        a, b, c = [float(g) for g in opt['gains']]
    except (TypeError, ValueError):
        raise ValueError('track: gains must be three numbers (a, b, c), got {!r}'.format(opt['gains']))
    if not (0.0 < a <= 1.0 and 0.0 <= b <= 1.0 and 0.0 <= c <= 1.0):
        raise ValueError('track: gains must satisfy 0 < a <= 1, 0 <= b <= 1, 0 <= c <= 1, got {!r}'.format((a, b, c)))
    if int(opt['max_age']) != opt['max_age'] or opt['max_age'] < 0:
        raise ValueError('track: max_age must be an integer >= 0, got {!r}'.format(opt['max_age']))
    birth = float(opt['birth_score'])
    if np.isnan(birth):
        raise ValueError('track: birth_score must not be NaN')
    assign = opt.get('assign', 'greedy')
    if not isinstance(assign, str) or assign not in ASSIGNS:
        raise ValueError("track: assign must be 'greedy' or 'optimal', got {!r}".format(assign))
    out = {'metric': opt['metric'], 'threshold': thr, 'max_age': int(opt['max_age']), 'gains': (a, b, c), 'birth_score': birth,
           'smooth': bool(opt['smooth'])}
    ego = opt.get('ego', False)
    if not isinstance(ego, (bool, np.bool_)):
        raise ValueError("track: ego must be True or False, got {!r}".format(ego))
    if assign == 'optimal':
        out['assign'] = assign
    if ego:
        out['ego'] = True
    if kind == 'kalman':
        out['filter'], out['noise'] = kind, noise
    return out


def empty_state(S=None):
    """ the empty tracker: one record (S None) or S of them """
    return np.zeros(() if S is None else (int(S),), STATE_DTYPE)


def read_state(buffer):
    """ the bytes of gpp_track_state(s) -- a uint8 tensor or array (S, bytes) or (bytes,), or a bytes object -> a STATE_DTYPE array (S,) or
    one record; a copy """
    if hasattr(buffer, 'cpu'):
        buffer = buffer.cpu().numpy()
    raw = np.frombuffer(buffer, np.uint8) if isinstance(buffer, (bytes, bytearray)) else np.ascontiguousarray(buffer).view(np.uint8)
    if raw.size % STATE_DTYPE.itemsize:
        raise ValueError('read_state: {} bytes are no multiple of a state ({})'.format(raw.size, STATE_DTYPE.itemsize))
    out = raw.reshape(-1).view(STATE_DTYPE).copy()
    return out[0] if np.ndim(buffer) <= 1 and out.size == 1 else out


def empty_cov(S=None):
    """ the covariances of the empty tracker: (10, MAX_TRACKS) float64 zeros (S None) or (S, 10, MAX_TRACKS) -- gpp_track_cov """
    return np.zeros((len(COV_FIELDS), MAX_TRACKS) if S is None else (int(S), len(COV_FIELDS), MAX_TRACKS))


def read_cov(buffer):
    """ the bytes of gpp_track_cov(s) -- a uint8 tensor or array (S, bytes) or (bytes,), a float64 one, or a bytes object -> a float64
    array (S, 10, MAX_TRACKS), or (10, MAX_TRACKS) for one record given without its leading axis; a copy """
    if hasattr(buffer, 'cpu'):
        buffer = buffer.cpu().numpy()
    raw = np.frombuffer(buffer, np.uint8) if isinstance(buffer, (bytes, bytearray)) else np.ascontiguousarray(buffer).view(np.uint8)
    one = len(COV_FIELDS) * MAX_TRACKS * 8
    if raw.size % one:
        raise ValueError('read_cov: {} bytes are no multiple of a covariance record ({})'.format(raw.size, one))
    out = raw.reshape(-1).view(np.float64).reshape(-1, len(COV_FIELDS), MAX_TRACKS).copy()
    return out[0] if np.ndim(buffer) <= 1 and out.shape[0] == 1 else out


def tracks_of(state):
    """ one state -> a list of dicts, one per occupied slot in slot order: slot, id, hits, misses, score and the ten fields """
    out = []
    for t in np.flatnonzero(state['id1'] != 0):
        rec = {'slot': int(t), 'id': int(state['id1'][t]) - 1, 'hits': int(state['hits'][t]), 'misses': int(state['misses'][t]),
               'score': float(state['score'][t])}
        rec.update({name: float(state['box'][k][t]) for k, name in enumerate(FIELDS)})
        out.append(rec)
    return out


def ego_records(poses):
    """ (N, 4, 4) or (N, 3, 4) transforms -- a point p in the previous frame's camera coordinates lies at R p + t in this frame's -- ->
    the (N, 16) float64 records of gpp_track_ego_f64: R row-major, t, dyaw = atan2(R02 - R20, R00 + R22) (exact for a rotation about
    the camera's Y axis, the nearest yaw otherwise), three zeros """
    poses = np.asarray(poses, np.float64)
    if poses.ndim != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
        raise ValueError('ego_records: poses must be (N, 4, 4) or (N, 3, 4), got {}'.format(poses.shape))
    out = np.zeros((poses.shape[0], EGO_FIELDS))
    out[:, 0:9] = poses[:, :3, :3].reshape(-1, 9)
    out[:, 9:12] = poses[:, :3, 3]
    out[:, 12] = np.arctan2(poses[:, 0, 2] - poses[:, 2, 0], poses[:, 0, 0] + poses[:, 2, 2])
    return check_ego(out, poses.shape[0])


def check_ego(ego, N):
    """ the records of N frames -> a C-contiguous (N, 16) float64 array; ValueError for another shape, a value that is not finite or a
    padding word that is not 0 (what gpp_track_ego_f64 refuses with GPP_ERR_BAD_ARG) """
    ego = np.ascontiguousarray(ego, np.float64)
    if ego.shape != (int(N), EGO_FIELDS):
        raise ValueError('track: ego must be ({}, {}) -- one record per frame --, got {}'.format(int(N), EGO_FIELDS, ego.shape))
    if not np.isfinite(ego).all():
        raise ValueError('track: an ego record holds a value that is not finite (frame {})'.format(int(np.argwhere(~np.isfinite(ego))[0][0])))
    if (ego[:, 13:] != 0.0).any():
        raise ValueError('track: the last three words of an ego record must be 0 (frame {})'.format(int(np.argwhere(ego[:, 13:] != 0.0)[0][0])))
    return ego


def row_noise(rows, noise):
    """ section 4.34, "row noise" (utils/track_kf.py): rows (D, 36) float32 -> (3, D) float64, Rxx Rxz Rzz of every row """
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        return KF.row_noise(rows[:, 19].astype(np.float64), rows[:, 21].astype(np.float64), noise)


def candidate_keys(box, occupied, rows, valid, metric, threshold, cov=None, noise=None):
    """ the candidate table of one frame: (MAX_TRACKS, D) float64, +inf where the pair is no candidate, otherwise its key -- the smaller
    the better: q for 'dist', m for 'maha' (cov (10, MAX_TRACKS): the PREDICTED covariance, noise (3, D): row_noise), minus the overlap
    otherwise.  box (10, MAX_TRACKS): the PREDICTED state; rows (D, 36) float32 """
    D = rows.shape[0]
    keys = np.full((MAX_TRACKS, D), np.inf)
    ts, ds = np.flatnonzero(occupied), np.flatnonzero(valid)
    if ts.size == 0 or ds.size == 0:
        return keys
    t, d = np.repeat(ts, ds.size), np.tile(ds, ts.size)
    g = rows[d].astype(np.float64)
    sx, sy, sz, sry, sh, sw, sl = [box[k][t] for k in range(7)]
    gx, gy, gz, gry, gh, gw, gl = [g[:, c] for c in ROW_COLS]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if metric == 'dist':
            dx, dz = gx - sx, gz - sz
            q = dx * dx + dz * dz
            hit = q < threshold * threshold
            keys[t[hit], d[hit]] = q[hit]
            return keys
        if metric == 'maha':
            dx, dz = gx - sx, gz - sz
            sxx, sxz, szz, det = KF.innovation(cov[:3, t], noise[:, d])
            m = ((((szz * dx) * dx) - ((2.0 * (sxz * dx)) * dz)) + ((sxx * dz) * dz)) / det
            hit = (det > 0.0) & (m < threshold * threshold)
            keys[t[hit], d[hit]] = m[hit]
            return keys
        inter = kitti_eval.rect_intersections(sl, sw, sx, sz, sry, gl, gw, gx, gz, gry)
        area_d, area_g = sl * sw, gl * gw
        if metric == 'bev':
            o = inter / (area_d + area_g - inter)
        else:
            iv = inter * kitti_eval.height_overlaps(sy, sh, gy, gh)
            o = iv / (area_d * sh + area_g * gh - iv)
        hit = o > threshold
    keys[t[hit], d[hit]] = -o[hit]
    return keys


def greedy(keys):
    """ candidates best first (ties: the smaller slot, then the smaller row), each taken iff its slot and its row are both still free
    -> [(slot, row)] in the order taken """
    t, d = np.nonzero(np.isfinite(keys))
    order = np.lexsort((d, t, keys[t, d]))
    slot_taken, row_taken, out = set(), set(), []
    for k in order:
        if t[k] in slot_taken or d[k] in row_taken:
            continue
        slot_taken.add(t[k])
        row_taken.add(d[k])
        out.append((int(t[k]), int(d[k])))
    return out


def cost_cells(keys, occupied, valid, metric, threshold):
    """ the matrix of section 4.32 from a frame's candidate table: (cost (n, n) int32 with n = max(T, R), the T occupied slots ascending
    -- the matrix's rows --, the R live, non-blind rows ascending -- its columns).  A candidate's cell lies in [0, SCALE - 1]:
    floor(q / threshold^2 * 2^20) for 'dist' (and 'maha', with m for q), 2^20 - floor(min(o * 2^20, 2^20)) otherwise; every other cell is SCALE """
    ts, ds = np.flatnonzero(occupied), np.flatnonzero(valid)
    n = max(ts.size, ds.size)
    cost = np.full((n, n), SCALE, np.int32)
    if ts.size and ds.size:
        sub = keys[np.ix_(ts, ds)]
        cand = np.isfinite(sub)
        value = np.where(cand, sub, 0.0)
        if metric in ('dist', 'maha'):
            t2 = threshold * threshold
            r = value / t2
            x = r * 1048576.0
            cell = np.minimum(np.floor(x), SCALE - 1)
        else:
            k = np.floor(np.minimum(-value * 1048576.0, 1048576.0))
            cell = np.minimum(SCALE - k, SCALE - 1)
        cost[:ts.size, :ds.size] = np.where(cand, cell, SCALE).astype(np.int32)
    return cost, ts, ds


def optimal(keys, occupied, valid, metric, threshold):
    """ the assignment of the least total over cost_cells' matrix (mot_eval.assign_np: rows in order, one shortest augmenting path each,
    ties to the first column); a slot and a row are matched iff they are assigned to each other AND are a candidate
    -> [(slot, row)] in slot order """
    cost, ts, ds = cost_cells(keys, occupied, valid, metric, threshold)
    if ts.size == 0 or ds.size == 0:                     # (every cell is SCALE: whatever is assigned, nothing is matched)
        return []
    col, _ = mot_eval.assign_np(cost)
    return [(int(ts[i]), int(ds[col[i]])) for i in range(ts.size) if col[i] < ds.size and cost[i, col[i]] < SCALE]


def step_np(state, rows, opt, keys_out=None, ego=None, cov=None):
    """ one frame step on `state` (one writable STATE_DTYPE record, changed in place) -> (rows_out (D, 36) float32, ids (D,) int32,
    hits (D,) int32).  keys_out: a list that receives the frame's candidate table (the tests' margins); ego: the frame's record (16,),
    checked by the caller (check_ego) -- step 1b of section 4.33; cov: with 'filter': 'kalman' the sequence's (10, MAX_TRACKS) float64
    covariances, changed in place (section 4.34; every expression is the specification's, one NumPy operation per float64 operation) """
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    D = rows.shape[0]
    if D > MAX_DETECTIONS:
        raise ValueError('track: {} rows in a frame, at most {}'.format(D, MAX_DETECTIONS))
    a, b, c = opt['gains']
    box, id1, hits, misses, score = state['box'], state['id1'], state['hits'], state['misses'], state['score']
    occupied = id1 != 0
    kalman = opt.get('filter') == 'kalman'
    if kalman:
        q_pos, q_vel = opt['noise']['process']
        speed = opt['noise']['birth_speed']
    box[0:3, occupied] = box[0:3, occupied] + box[7:10, occupied]                                  # 1 predict
    if kalman:
        cov[:, occupied] = KF.predict_cov(cov[:, occupied], q_pos, q_vel)
    if ego is not None:                                                                             # 1b ego
        # the products are written out, one NumPy operation per float64 operation of the rule and in its association: `@`, dot and
        # einsum go through BLAS, which may fuse a multiply with an add or sum in another order
        e = [float(v) for v in np.asarray(ego, np.float64).reshape(EGO_FIELDS)]
        x, y, z = box[0, occupied].copy(), box[1, occupied].copy(), box[2, occupied].copy()
        vx, vy, vz = box[7, occupied].copy(), box[8, occupied].copy(), box[9, occupied].copy()
        for k in range(3):
            box[k, occupied] = ((e[3 * k] * x + e[3 * k + 1] * y) + e[3 * k + 2] * z) + e[9 + k]
            box[7 + k, occupied] = (e[3 * k] * vx + e[3 * k + 1] * vy) + e[3 * k + 2] * vz
        box[3, occupied] = wrap(box[3, occupied] + e[12])
        if kalman:                                                                                  # (the ground part of R on every block)
            cov[:, occupied] = KF.turn_cov(cov[:, occupied], (e[0], e[2], e[6], e[8]))
    live = rows[:, 14] >= 0.0                                                                       # 2 rows
    valid = live & ~np.isnan(rows[:, ROW_COLS]).any(axis=1)
    noise = row_noise(rows, opt['noise']) if kalman else None
    keys = candidate_keys(box, occupied, rows, valid, opt['metric'], opt['threshold'], cov, noise)  # 3 candidates
    if keys_out is not None:
        keys_out.append(keys)
    if opt.get('assign') == 'optimal':                                                              # 4 greedy, or section 4.32's assignment
        pairs = optimal(keys, occupied, valid, opt['metric'], opt['threshold'])
    else:
        pairs = greedy(keys)
    row_slot = np.full(D, -1, np.int64)
    if pairs:                                                                                       # 5 update
        t, d = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        z = rows[d][:, ROW_COLS].astype(np.float64).T                                               # (7, matched)
        r = z[0:3] - box[0:3, t]
        if kalman:
            R = noise[:, d]
            with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
                mean, new, good = KF.update(box[[0, 2, 7, 9]][:, t], cov[:, t], R, r[0], r[2])
            cov[:, t] = np.where(good, new, KF.born_cov(R, speed))                                  # det not > 0: the fixed gains, P as at birth
        box[7:10, t] = box[7:10, t] + b * r
        box[0:3, t] = box[0:3, t] + a * r
        if kalman:
            for k, m in zip((0, 2, 7, 9), mean):
                box[k, t] = np.where(good, m, box[k, t])
        box[4:7, t] = box[4:7, t] + c * (z[4:7] - box[4:7, t])
        delta = wrap(z[3] - box[3, t])
        delta = np.where(delta >= PI / 2.0, delta - PI, delta)
        delta = np.where(delta < -(PI / 2.0), delta + PI, delta)
        box[3, t] = wrap(box[3, t] + a * delta)
        hits[t] += 1
        misses[t] = 0
        score[t] = rows[d, 12]
        row_slot[d] = t
    lost = occupied.copy()                                                                          # 6 deaths
    lost[[p[0] for p in pairs]] = False
    misses[lost] += 1
    dead = lost & (misses > opt['max_age'])
    for field in (id1, hits, misses, score):
        field[dead] = 0
    box[:, dead] = 0.0
    if kalman:
        cov[:, dead] = 0.0
    with np.errstate(invalid='ignore'):                                                             # 7 births
        born = np.flatnonzero(valid & (row_slot < 0) & (rows[:, 12].astype(np.float64) >= opt['birth_score']))
    free = np.flatnonzero(id1 == 0)
    n = min(born.size, free.size)
    t, d = free[:n], born[:n]
    id1[t] = state['next_id'] + np.arange(n, dtype=np.int32) + 1
    hits[t], misses[t], score[t] = 1, 0, rows[d, 12]
    box[0:7, t] = rows[d][:, ROW_COLS].astype(np.float64).T
    box[7:10, t] = 0.0
    if kalman:
        cov[:, t] = KF.born_cov(noise[:, d], speed)
    row_slot[d] = t
    state['next_id'] += n
    state['dropped'] += born.size - n
    state['frames'] += 1
    has = row_slot >= 0                                                                             # 8 outputs
    ids = np.where(has, id1[row_slot] - 1, -1).astype(np.int32)
    out_hits = np.where(has, hits[row_slot], 0).astype(np.int32)
    out = rows.copy()
    if opt['smooth'] and has.any():
        t = row_slot[has]
        for k, col in enumerate(ROW_COLS):
            out[has, col] = box[k, t].astype(np.float32)
        out[has, 25] = wrap(box[3, t] - np.arctan2(box[0, t], box[2, t])).astype(np.float32)
    return out, ids, out_hits


def track_rows_np(rows_per_frame, options, state=None, keys_out=None, ego=None, cov=None):
    """ the NumPy form: rows_per_frame (N, D, 36) float32 (or a list of (D_f, 36) arrays), the consecutive frames of one sequence; options:
    what check_option takes; state: one STATE_DTYPE record (None: the empty tracker; it is not changed) -> (rows_out, ids, hits, state):
    arrays (N, D, 36), (N, D), (N, D) (lists for a list) and the new state.  As the device form, N * D == 0 leaves the state as it is.
    ego: None, or the (N, 16) records of the frames (ego_records; section 4.33); the first relates to the last frame `state` has seen.
    With 'filter': 'kalman' (section 4.34) the result has a fifth member, the new (10, MAX_TRACKS) covariances; cov: those that belong to
    `state` (None: zeros, the empty tracker's; not changed).  Without the filter `cov` must be None. """
    opt = check_option(options)
    kalman = opt.get('filter') == 'kalman'
    if cov is not None and not kalman:
        raise ValueError("track: a covariance was given, but the option has no 'filter': 'kalman'")
    if kalman:
        cov = empty_cov() if cov is None else np.array(cov, np.float64).reshape(len(COV_FIELDS), MAX_TRACKS)
    more = (cov,) if kalman else ()
    if ego is not None:
        ego = check_ego(ego, len(rows_per_frame))
    state = empty_state() if state is None else np.array(state, STATE_DTYPE).reshape(())
    state = state.copy()
    as_list = isinstance(rows_per_frame, (list, tuple))
    frames = [np.asarray(r, np.float32).reshape(-1, POSE_COLS) for r in rows_per_frame] if as_list else np.asarray(rows_per_frame, np.float32)
    if not as_list and frames.size == 0:
        return (frames.copy(), np.zeros(frames.shape[:2], np.int32), np.zeros(frames.shape[:2], np.int32), state) + more
    res = [step_np(state, r, opt, keys_out, None if ego is None else ego[f], cov) for f, r in enumerate(frames)]
    if as_list:
        return ([x[0] for x in res], [x[1] for x in res], [x[2] for x in res], state) + more
    return (np.stack([x[0] for x in res]), np.stack([x[1] for x in res]), np.stack([x[2] for x in res]), state) + more


def params_of(options):
    """ options -> backend.hip.TrackParams """
    from ..backend import hip
    opt = check_option(options)
    a, b, c = opt['gains']
    return hip.TrackParams(metric_code(opt['metric'], opt.get('filter') == 'kalman'), opt['max_age'], int(opt['smooth']), 0, opt['threshold'], a, b, c, opt['birth_score'])


def kf_params_of(options):
    """ options -> backend.hip.TrackKfParams, or None without 'filter': 'kalman' """
    from ..backend import hip
    opt = check_option(options)
    if opt.get('filter') != 'kalman':
        return None
    n = opt['noise']
    return hip.TrackKfParams(n['radial'][0], n['radial'][1], n['tangential'][0], n['tangential'][1], n['process'][0], n['process'][1],
                             n['birth_speed'], 0)


def cov_tensor(cov, device, S=1):
    """ None (S empty trackers), float64 covariances (10, MAX_TRACKS) / (S, 10, MAX_TRACKS) or a uint8 tensor -> the (S, bytes) uint8
    tensor gpp_track_kf_f64 takes """
    import torch
    if isinstance(cov, torch.Tensor):
        return cov
    host = empty_cov(S) if cov is None else np.ascontiguousarray(cov, np.float64).reshape(-1, len(COV_FIELDS), MAX_TRACKS)
    return torch.as_tensor(host.view(np.uint8).reshape(host.shape[0], -1).copy()).to(device)


def add_filter_arguments(parser):
    """ the command lines' arguments of section 4.34 (bin/run_network.py, bin/track_results.py) """
    parser.add_argument('--track-filter', choices=list(FILTERS), default='fixed',
                        help='fixed: the fixed gains (section 4.28).  kalman: every track keeps the covariance of its ground-plane position and '
                             'velocity (gpp_track_kf_f64, DESIGN.md section 4.34); needs --track-noise, --track-process and --track-birth-speed '
                             '-- there are no defaults: nothing here has seen a real sequence.')
    parser.add_argument('--track-noise', type=float, nargs=4, default=None, metavar=('R0', 'R1', 'T0', 'T1'),
                        help='With --track-filter kalman: a detection at range rho has the standard deviation R0 + R1 rho metres along its '
                             'viewing ray and T0 + T1 rho across it.')
    parser.add_argument('--track-process', type=float, nargs=2, default=None, metavar=('QP', 'QV'),
                        help='With --track-filter kalman: the process variances of position and velocity per frame step.')
    parser.add_argument('--track-birth-speed', type=float, default=None, metavar='V0',
                        help='With --track-filter kalman: the standard deviation of a new track\'s velocity, metres per frame.')


def filter_option(args):
    """ add_filter_arguments' values -> the option's {'filter', 'noise'} entries ({} for 'fixed'); ValueError for a half-given filter """
    given = [args.track_noise is not None, args.track_process is not None, args.track_birth_speed is not None]
    if args.track_filter != 'kalman':
        if any(given):
            raise ValueError('--track-noise, --track-process and --track-birth-speed belong to --track-filter kalman')
        return {}
    if not all(given):
        raise ValueError('--track-filter kalman needs --track-noise R0 R1 T0 T1, --track-process QP QV and --track-birth-speed V0 (no defaults)')
    return {'filter': 'kalman', 'noise': {'radial': tuple(args.track_noise[:2]), 'tangential': tuple(args.track_noise[2:]),
                                         'process': tuple(args.track_process), 'birth_speed': args.track_birth_speed}}


def is_optimal(options):
    """ whether the option asks for gpp_track_optimal_f64 (the entry point, not a field of the parameters, carries the choice) """
    return check_option(options).get('assign') == 'optimal'


def state_tensor(state, device, S=1):
    """ None (S empty trackers), STATE_DTYPE records or a uint8 tensor -> the (S, bytes) uint8 tensor gpp_track_f64 takes """
    import torch
    if isinstance(state, torch.Tensor):
        return state
    host = empty_state(S) if state is None else np.atleast_1d(np.array(state, STATE_DTYPE))
    return torch.as_tensor(np.ascontiguousarray(host).view(np.uint8).reshape(host.shape[0], STATE_DTYPE.itemsize).copy()).to(device)


def track_rows_device(rows, options, state=None, seq_start=None, out=None, state_out=None, ego=None, cov=None, cov_out=None):
    """ csrc/track.hip (gpp_track_f64, or gpp_track_optimal_f64 for 'assign': 'optimal'): rows (N, D, 36), the frames of S sequences
    (seq_start (S + 1,), default one sequence of all frames): a NumPy array
    -> NumPy results and STATE_DTYPE state(s), or a float32 device tensor -> device tensors with the state as (S, bytes) uint8 (no
    synchronisation; read_state reads it).  state: None (empty), STATE_DTYPE record(s) or such a tensor.  out / state_out (tensors only):
    where the rows and the state go -- `rows` and `state` themselves are allowed.  ego: None, or the (N, 16) HOST records of the frames
    (section 4.33): gpp_track_ego_f64 with the option's assignment.
    With 'filter': 'kalman' (section 4.34) the launch is gpp_track_kf_f64, with or without records: cov: the covariances that belong to
    `state` -- None (zeros), float64 (10, 128) / (S, 10, 128) or an (S, bytes) uint8 tensor --, cov_out (tensors only): where they go,
    `cov` itself allowed; the result has a fifth member, the new covariances (float64 arrays, or the uint8 tensor: read_cov reads it).
    Returns (rows_out, ids (N, D) int32, hits (N, D) int32, state).  D <= 128. """
    import torch
    from ..backend import hip
    params, best, kf = params_of(options), is_optimal(options), kf_params_of(options)
    if kf is None and (cov is not None or cov_out is not None):
        raise ValueError("track: a covariance was given, but the option has no 'filter': 'kalman'")
    S = 1 if seq_start is None else len(seq_start) - 1
    if ego is not None:
        ego = check_ego(ego, len(rows))
    if isinstance(rows, torch.Tensor):
        if rows.dim() != 3 or not rows.is_contiguous():
            raise ValueError('track_rows_device: rows must be a dense (N, D, {}) tensor, got {}'.format(POSE_COLS, tuple(rows.shape)))
        more = {} if kf is None else {'kf': kf, 'cov_in': cov_tensor(cov, rows.device, S), 'cov_out': cov_out}
        return hip.track(rows, state_tensor(state, rows.device, S), params, seq_start, state_out=state_out, out=out, optimal=best, ego=ego, **more)
    host = np.ascontiguousarray(rows, np.float32)
    if host.ndim != 3 or host.shape[2] != POSE_COLS:
        raise ValueError('track_rows_device: rows must be (N, D, {}), got {}'.format(POSE_COLS, host.shape))
    dev = hip.require_device()
    more = {} if kf is None else {'kf': kf, 'cov_in': cov_tensor(cov, dev, S)}
    res = hip.track(torch.as_tensor(host).to(dev), state_tensor(state, dev, S), params, seq_start, optimal=best, ego=ego, **more)
    new = read_state(res[3])
    result = res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy(), (new[0] if seq_start is None else new)
    if kf is not None:
        new_cov = read_cov(res[4])
        result += ((new_cov[0] if seq_start is None else new_cov),)
    return result


def tracking_lines(frame, rows, ids, hits, min_hits=1):
    """ the lines of one frame in KITTI's tracking format, `frame id Car -1 -1 alpha x1 y1 x2 y2 h w l x y z r_y score`: the rows that
    carry an id whose track has at least min_hits hits, in row order """
    rows = np.asarray(rows, np.float32).reshape(-1, POSE_COLS)
    ids, hits = np.asarray(ids).reshape(-1), np.asarray(hits).reshape(-1)
    keep = np.flatnonzero((ids >= 0) & (hits >= min_hits))
    values = rows[keep][:, gpp_utils.KITTI_COLUMNS].astype(np.float64)
    out = []
    for k, v in zip(keep, values):
        out.append(TRACKING_FORMAT % ((int(frame), int(ids[k])) + tuple(v.tolist())))
    return ''.join(out)


def id_switches(gt_ids_per_frame, ids_per_frame):
    """ the identity switches of a sequence: gt_ids_per_frame[f][k] is the true object of row k of frame f (< 0: none), ids_per_frame[f][k]
    the id the tracker gave it (< 0: none).  A switch is counted whenever an object carries another id than the last one it carried. """
    last, switches = {}, 0
    for gts, ids in zip(gt_ids_per_frame, ids_per_frame):
        for g, i in zip(np.asarray(gts).reshape(-1).tolist(), np.asarray(ids).reshape(-1).tolist()):
            if g < 0 or i < 0:
                continue
            if g in last and last[g] != i:
                switches += 1
            last[g] = i
    return switches
