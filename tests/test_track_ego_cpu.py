""" CPU tests of the tracker's ego-motion compensation: the NumPy form (utils/track.py, `ego`) against the
loop-written oracle (tests/track_ego_oracle.py) for both assignments and all three metrics; the margins that let
tests/test_track_ego_gpu.py ask for equality; what the step is for -- a parked car keeps its id from a driving camera --; identity
records, chunked calls, the option and the records' checks; the C ABI's argument checks (host code: they come before any launch). """
import ctypes
import re

import numpy as np
import pytest

import track_ego_oracle as E
import track_optimal_oracle as P
import track_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import track as T

EXACT = E.exact_cases()
MARGIN = E.margin_cases()
ids_of = lambda cases: [c[0] for c in cases]  # noqa: E731
SCENES = {'curve': E.curve, 'pitching': E.pitching, 'straight': E.straight, 'with_movers': E.with_movers}


def same_as_oracle(frames, ego, opt, state=None, values=None):
    want_rows, want_ids, want_hits, want_state = E.track(frames, opt, ego, values=values)
    got_rows, got_ids, got_hits, got_state = T.track_rows_np(frames, opt, ego=ego)
    assert got_rows.dtype == np.float32 and got_ids.dtype == np.int32 and got_hits.dtype == np.int32
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_hits, want_hits)
    assert O.same_state(want_state, got_state)                                    # every field, ==
    cols = [c for c in range(36) if c != 25 or not opt['smooth']]
    assert np.array_equal(got_rows[..., cols], want_rows[..., cols], equal_nan=True)          # (numeric: see the oracle's docstring on -0.0)
    close = np.abs(got_rows[..., 25].astype(np.float64) - want_rows[..., 25]) <= 4 * np.spacing(np.abs(want_rows[..., 25]))
    assert (close | (got_rows[..., 25] == want_rows[..., 25])).all()
    return got_ids, got_state


def optimal_gaps(frames, ego, opt):
    """ section 4.32's gap per frame with a matched pair: (second-best total) - (best total) - 2 * (matched pairs), by brute force over
    the oracle's own matrices: the best total with one matched candidate forbidden """
    from scipy.optimize import linear_sum_assignment
    matrices = []
    E.track(frames, opt, ego, matrices=matrices)

    def total(cost):
        cost = np.asarray(cost, np.int64).reshape(len(cost), len(cost))
        r, c = linear_sum_assignment(cost)
        return int(cost[r, c].sum())

    gaps = []
    for cost, slots, rows, pairs in matrices:
        if not pairs:
            continue
        best, second = total(cost), None
        for t, d in pairs:
            forbidden = np.array(cost, np.int64)
            forbidden[slots.index(t), rows.index(d)] = P.S
            second = total(forbidden) if second is None else min(second, total(forbidden))
        gaps.append(second - best - 2 * len(pairs))
    return gaps


@pytest.mark.parametrize('name,frames,ego,opt', EXACT, ids=ids_of(EXACT))
def test_host_form_equals_the_oracle_on_the_exact_cases(name, frames, ego, opt):
    values = []
    ids, state = same_as_oracle(frames, ego, opt, values=values)
    to_thr, _ = O.margins(values, opt)
    assert to_thr > 1e-9, to_thr                       # (no candidate sits on the threshold; equal candidates are wanted here)
    # the carried scene is tracked as the standing one is: the records cancel the camera's motion exactly
    plain = name.rsplit('_', 2)[0]
    scene = {'crossing': O.crossing(), 'crossing_smooth': O.crossing(), 'gap_max_age': O.gap(2), 'gap_max_age_plus_1': O.gap(3),
             'tie_rows': O.tie_rows(), 'tie_slots': O.tie_slots()}[plain]
    _, still_ids, _, still_state = T.track_rows_np(scene, opt)
    assert np.array_equal(ids, still_ids) and int(state['next_id']) == int(still_state['next_id'])


def test_the_tie_cases_do_tie():
    """ the carried tie scenes still hold two equal candidates in frame 1, and the rule's tie-break decides """
    for name, frames, ego, opt in EXACT:
        if not name.startswith('tie_'):
            continue
        values = []
        E.track(frames, opt, ego, values=values)
        assert len(values[1]) == 2 and values[1][0][0] == values[1][1][0], (name, values[1])
        ids = T.track_rows_np(frames, opt, ego=ego)[1]
        assert ids.tolist() == ([[0, -1], [0, 1]] if name.startswith('tie_rows') else [[0, 1], [0, -1]]), name


@pytest.mark.parametrize('name,frames,ego,opt', MARGIN, ids=ids_of(MARGIN))
def test_host_form_equals_the_oracle_where_the_margins_hold(name, frames, ego, opt):
    """ what lets the GPU test ask for equality: section 4.28's margins -- no value within 1e-9 of the threshold, no two candidates of a
    frame within 1e-9 of each other -- and, for 'optimal', section 4.32's gap: the best total is alone by more than 2 * (matched pairs) """
    values = []
    same_as_oracle(frames, ego, opt, values=values)
    to_thr, apart = O.margins(values, opt)
    print(name, 'to the threshold', to_thr, 'between candidates', apart)
    assert to_thr > 1e-9 and apart > 1e-9, (to_thr, apart)
    if opt.get('assign') == 'optimal':
        gaps = optimal_gaps(frames, ego, opt)
        print(name, 'min(gap - 2 pairs) =', min(gaps))
        assert gaps and min(gaps) > 0


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric,thr', E.FOR)
@pytest.mark.parametrize('scene', sorted(SCENES))
def test_parked_cars_keep_their_ids_from_a_driving_camera(scene, metric, thr, assign):
    """ what the step is for.  Without records the ego step of every frame tears the tracks (more ids than cars; on the curve a new id
    for every row); with them there is one id per car, no switch, and a parked car's velocity stays far below the 1.5 m the camera
    moves per frame (0.1 m/frame: the oracle's largest component is 0.021 on these scenes) """
    frames, ego, gts = SCENES[scene]()
    opt = dict(O.options(metric, thr), **({'assign': 'optimal'} if assign == 'optimal' else {}))
    _, plain_ids, _, plain_state = T.track_rows_np(frames, opt)
    assert int(plain_state['next_id']) > E.CARS and len(set(plain_ids[plain_ids >= 0].tolist())) > E.CARS
    _, ids, hits, state = T.track_rows_np(frames, opt, ego=ego)
    assert int(state['next_id']) == E.CARS and sorted(set(ids[ids >= 0].tolist())) == list(range(E.CARS))
    assert T.id_switches(gts, ids) == 0 and (ids >= 0).sum() == E.CARS * len(frames) and hits.max() == len(frames)
    parked = [int(np.flatnonzero(state['id1'] == ids[0][list(gts[0]).index(k)] + 1)[0]) for k in range(2 if scene == 'with_movers' else 0, E.CARS)]
    assert np.abs(state['box'][7:10][:, parked]).max() < 0.1
    if scene == 'with_movers':                         # the two that do move 0.4 m/frame: the velocity is their own, in the last camera's
        moving = [int(np.flatnonzero(state['id1'] == ids[0][list(gts[0]).index(k)] + 1)[0]) for k in range(2)]      # axes (the filter
        speed = np.sqrt((state['box'][7:10][:, moving] ** 2).sum(axis=0))          # started them at 0 eleven updates ago and still converges)
        assert ((speed > 0.2) & (speed < 0.6)).all(), speed


def test_the_issue_s_numbers():
    """ the curve: 96 ids for 8 cars (a new id for every row of every frame) under three of the options and 49 under ('dist', 2.0);
    straight ahead at 2.5 m/frame 42; 8 with records; the largest velocity component 0.021 m/frame """
    frames, ego, _ = E.curve()
    counts = {(m, t): int(T.track_rows_np(frames, O.options(m, t))[3]['next_id']) for m, t in E.FOR}
    assert counts == {('dist', 1.0): 96, ('dist', 2.0): 49, ('bev', 0.25): 96, ('3d', 0.25): 96}
    state = T.track_rows_np(frames, O.options('dist', 1.0), ego=ego)[3]
    assert int(state['next_id']) == 8 and round(float(np.abs(state['box'][7:10]).max()), 3) == 0.021
    frames, ego, _ = E.straight()
    assert int(T.track_rows_np(frames, O.options('dist', 1.0))[3]['next_id']) == 42
    assert int(T.track_rows_np(frames, O.options('dist', 1.0), ego=ego)[3]['next_id']) == 8


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric', T.METRICS)
def test_identity_records_change_nothing(metric, assign):
    """ R = I, t = 0, dyaw = 0: the ids and hits of ego=None and every state field equal with == ((-0.0) + 0.0 may change a zero's
    sign: no bytes are compared) """
    frames = O.drive(O.DRIVE_SEED)
    opt = dict(O.options(metric, smooth=True), **({'assign': 'optimal'} if assign == 'optimal' else {}))
    ego = np.array([E.IDENTITY] * len(frames))
    want, got = T.track_rows_np(frames, opt), T.track_rows_np(frames, opt, ego=ego)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0], equal_nan=True)
    for field in T.STATE_DTYPE.names:
        assert np.array_equal(got[3][field], want[3][field]), field
    assert (want[1] >= 0).sum() > 40


@pytest.mark.parametrize('assign', T.ASSIGNS)
def test_any_cut_into_calls_gives_the_same_result(assign):
    """ every cut of the curve into two calls, and one into four, each call with its slice of the records: the record of a call's first
    frame relates to the last frame of the call before """
    frames, ego, _ = E.curve()
    opt = dict(O.options('bev', 0.25, smooth=True), **({'assign': 'optimal'} if assign == 'optimal' else {}))
    whole = T.track_rows_np(frames, opt, ego=ego)
    for cuts in [[0, c, len(frames)] for c in range(1, len(frames))] + [[0, 1, 4, 9, len(frames)]]:
        state, parts = None, []
        for a, b in zip(cuts, cuts[1:]):
            r, i, h, state = T.track_rows_np(frames[a:b], opt, state, ego=ego[a:b])
            parts.append((r, i, h))
        for k in range(3):
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes()
        assert state.tobytes() == whole[3].tobytes()


def test_list_input_and_the_empty_call():
    frames, ego, _ = E.curve()
    opt = O.options('dist', 1.0)
    whole = T.track_rows_np(frames, opt, ego=ego)
    as_list = T.track_rows_np(list(frames), opt, ego=ego)
    assert isinstance(as_list[1], list) and np.array_equal(np.stack(as_list[1]), whole[1]) and as_list[3].tobytes() == whole[3].tobytes()
    empty = T.track_rows_np(np.zeros((0, 16, 36), np.float32), opt, whole[3], ego=np.zeros((0, 16)))
    assert empty[3].tobytes() == whole[3].tobytes()


# ---------------------------------------------------------------------------------------------------- options and records
def test_check_option_takes_ego():
    base = {'metric': 'dist', 'threshold': 2.0}
    assert T.check_option(dict(base, ego=True)) == dict(T.DEFAULTS, ego=True, **base)
    assert T.check_option(dict(base, ego=False)) == dict(T.DEFAULTS, **base) and 'ego' not in T.check_option(dict(base, ego=False))
    both = T.check_option(dict(base, ego=True, assign='optimal'))
    assert both == dict(T.DEFAULTS, ego=True, assign='optimal', **base) and T.check_option(both) == both and T.is_optimal(both)
    for bad in ('yes', 1, 0, None, 'True'):
        with pytest.raises(ValueError, match='ego'):
            T.check_option(dict(base, ego=bad))
    # the round trips without 'ego' are what they were
    assert 'ego' not in T.DEFAULTS and T.check_option(('bev', 0)) == dict(T.DEFAULTS, metric='bev', threshold=0.0)
    full = {'metric': 'dist', 'threshold': 2.0, 'max_age': 0, 'gains': (1.0, 0.0, 1.0), 'birth_score': -1.0, 'smooth': True}
    assert T.check_option(full) == full and T.check_option(T.check_option(full)) == full
    once = T.check_option(dict(base, assign='optimal'))
    assert once == dict(T.DEFAULTS, assign='optimal', **base) and T.check_option(once) == once
    p, q = T.params_of(dict(base, ego=True)), T.params_of(base)                    # the parameters carry nothing of it
    assert bytes(p) == bytes(q)


def test_check_ego_and_ego_records():
    good = np.array([E.IDENTITY, E.TURNS[0]])
    assert T.check_ego(good, 2).tobytes() == good.tobytes() and T.check_ego(good.tolist(), 2).dtype == np.float64
    for bad, n in ((good, 3), (good[:, :13], 2), (good.reshape(-1), 2), (good[None], 2)):
        with pytest.raises(ValueError, match='one record per frame'):
            T.check_ego(bad, n)
    for value in (np.nan, np.inf, -np.inf):
        for k in (0, 9, 12, 15):
            bad = good.copy()
            bad[1, k] = value
            with pytest.raises(ValueError, match='not finite'):
                T.check_ego(bad, 2)
    for k in (13, 14, 15):
        bad = good.copy()
        bad[0, k] = 1e-300
        with pytest.raises(ValueError, match='must be 0'):
            T.check_ego(bad, 2)
    with pytest.raises(ValueError):
        T.track_rows_np(O.crossing(), O.options('dist'), ego=good)                 # 9 frames, 2 records
    # ego_records: R, t and the yaw of a rotation about Y, exactly where R is a signed permutation
    poses = np.zeros((3, 4, 4))
    poses[:, 3, 3] = 1.0
    poses[0, :3, :3], poses[1, :3, :3], poses[2, :3, :3] = E.LEFT, E.BACK, E.rot_y(0.04)[:3, :3]
    poses[:, :3, 3] = [[0.5, 0.125, -0.25], [0.25, 0.0, -3.0], [0.0, 0.0, -1.5]]
    rec = T.ego_records(poses)
    assert rec.shape == (3, 16) and rec.dtype == np.float64 and (rec[:, 13:] == 0.0).all()
    assert rec[0].tolist() == E.TURNS[0] and rec[1].tolist() == E.TURNS[3]         # dyaw: the same doubles, pi / 2 and pi
    assert abs(rec[2, 12] - 0.04) < 1e-15
    assert T.ego_records(poses[:, :3]).tobytes() == rec.tobytes()
    tilted = poses[2:].copy()
    tilted[0, :3, :3] = E.rot_y(0.04).dot(E.rot_x(0.01))[:3, :3]                   # pitch: the nearest yaw
    assert abs(T.ego_records(tilted)[0, 12] - 0.04) < 1e-5
    for bad in (poses[0], poses[:, :2], np.zeros((3, 4, 3))):
        with pytest.raises(ValueError, match='ego_records'):
            T.ego_records(bad)
    poses[1, 0, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        T.ego_records(poses)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_contract():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'gpp.h')).read()
    contract = text[text.index('Tracking with EGO-MOTION compensation'):text.index('int gpp_track_ego_f64(')]
    contract = ' '.join(re.sub(r'\n \*', ' ', contract).split())
    for phrase in ("x' = ((R00 x + R01 y) + R02 z) + t0", "vx' = (R00 vx + R01 vy) + R02 vz", "r_y' = wrap(r_y + dyaw)", 'on the HOST',
                   'atan2(R02 - R20, R00 + R22)', 'three words that must be 0', 'GPP_TRACK_EGO_FIELDS 16', 'With an empty tracker a record has no effect',
                   'neither checked nor read', '128 bytes per frame', 'r_y only takes the yaw'):
        assert phrase in contract, phrase
    assert T.EGO_FIELDS == hip.GPP_TRACK_EGO_FIELDS == E.FIELDS == 16


def ego_call(ego, assign=0, N=4, seq=(0, 4), params=None):
    """ host code: every device pointer is null -- a refusal returns before it is looked at """
    good = hip.TrackParams(2, 2, 0, 0, 2.0, 0.5, 0.25, 0.25, 0.0) if params is None else params
    seq = (ctypes.c_int32 * len(seq))(*seq)
    ptr = None if ego is None else np.ascontiguousarray(ego, np.float64).ctypes.data_as(ctypes.c_void_p)
    return hip.lib().gpp_track_ego_f64(None, N, 4, seq, len(seq) - 1, None, None, ctypes.byref(good), ptr, assign, None, None, None, None, 0, None)


def test_c_abi_refuses_bad_records_before_any_launch():
    good = np.array([E.IDENTITY] * 4)
    # a good call gets as far as the missing states: that refusal is gpp_track_f64's own and comes behind the records' checks
    assert ego_call(good) == -1 and ego_call(good, seq=(0,)) == 0                  # S == 0: GPP_OK
    assert ego_call(None) == -1 and ego_call(None, seq=(0,)) == -1                 # a null ego when N > 0, even without a sequence
    assert ego_call(None, N=0, seq=(0,)) == 0
    for assign in (-1, 2, 7):
        assert ego_call(good, assign, seq=(0,)) == -1
    for assign in (0, 1):
        assert ego_call(good, assign, seq=(0,)) == 0
    # with D = 129 a good call is GPP_ERR_UNSUPPORTED (-4), which comes behind the records' checks: -1 then means the record
    def code(ego, seq=(0, 4)):
        s = (ctypes.c_int32 * len(seq))(*seq)
        p = hip.TrackParams(2, 2, 0, 0, 2.0, 0.5, 0.25, 0.25, 0.0)
        return hip.lib().gpp_track_ego_f64(None, 4, 129, s, len(seq) - 1, None, None, ctypes.byref(p),
                                           ego.ctypes.data_as(ctypes.c_void_p), 0, None, None, None, None, 0, None)
    assert code(good) == -4
    for k in range(16):
        for value in ((np.nan, np.inf, -np.inf) if k < 13 else (np.nan, 1.0, -1e-300)):
            bad = good.copy()
            bad[2, k] = value
            assert code(bad) == -1, (k, value)
            assert code(bad, (0, 2, 2)) == -4 and code(bad, (3, 4)) == -4          # frame 2 outside every sequence: not checked
            assert code(bad, (0, 1, 3)) == -1
    n = ctypes.c_size_t(0)
    for S, N in ((1, 0), (1, 12), (3, 5), (0, 7)):
        assert hip.lib().gpp_track_ego_workspace_bytes(S, N, ctypes.byref(n)) == 0
        assert n.value == hip.track_workspace_bytes(S) + 128 * N == hip.track_ego_workspace_bytes(S, N) and n.value % 8 == 0
    assert hip.lib().gpp_track_ego_workspace_bytes(-1, 1, ctypes.byref(n)) == -1 and hip.lib().gpp_track_ego_workspace_bytes(1, -1, ctypes.byref(n)) == -1
    assert hip.lib().gpp_track_ego_workspace_bytes(1, 1, None) == -1
