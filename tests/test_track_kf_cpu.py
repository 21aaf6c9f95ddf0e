""" CPU tests of the tracker's Kalman filter: the NumPy form (utils/track.py, 'filter': 'kalman') against the
loop-written oracle (tests/track_kf_oracle.py) for both assignments, all four metrics, with and without ego records and in any
chunking; the margins that let tests/test_track_kf_gpu.py ask for equality; the demonstration scene no fixed threshold gets right; a
car born moving; 200 matched updates; the quarter turn of a covariance; a caller's covariance that is not positive definite; the
option's checks; the C ABI's argument checks (host code: they come before any launch). """
import ctypes
import os
import re

import numpy as np
import pytest

import track_ego_oracle as E
import track_kf_oracle as K
import track_optimal_oracle as P
import track_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import track as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()
AXX, AXZ, AZZ, BXX, BXZ, BZX, BZZ, CXX, CXZ, CZZ = range(10)


def same_as_oracle(frames, ego, opt, state=None, cov=None, **receive):
    """ ids, hits, every state field and every covariance word: ==; column 25 of smoothed rows (atan2) within 4 float32 ulp """
    oracle_state = None if state is None else state_for_oracle(state)
    want = K.track(frames, opt, ego, oracle_state, None if cov is None else cov.tolist(), **receive)
    got = T.track_rows_np(frames, opt, state, ego=ego, cov=cov)
    assert len(got) == 5 and got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert got[4].dtype == np.float64 and got[4].shape == (10, 128)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert O.same_state(want[3], got[3])
    assert K.same_cov(want[4], got[4])
    cols = [c for c in range(36) if c != 25 or not opt['smooth']]
    assert np.array_equal(got[0][..., cols], want[0][..., cols], equal_nan=True)
    close = np.abs(got[0][..., 25].astype(np.float64) - want[0][..., 25]) <= 4 * np.spacing(np.abs(want[0][..., 25]))
    assert (close | (got[0][..., 25] == want[0][..., 25])).all()
    return got


def state_for_oracle(record):
    st = {k: record[k].tolist() for k in ('id1', 'hits', 'misses', 'score', 'box')}
    st.update({k: int(record[k]) for k in ('next_id', 'frames', 'dropped')})
    return st


def optimal_gaps(matrices):
    """ section 4.32's gap per frame with a matched pair: (second-best total) - (best total) - 2 * (matched pairs), by brute force over
    the oracle's own matrices (tests/test_track_ego_cpu.py) """
    from scipy.optimize import linear_sum_assignment

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


# ---------------------------------------------------------------------------------------------------- the three forms
@pytest.mark.parametrize('name,frames,ego,opt', CASES, ids=[c[0] for c in CASES])
def test_numpy_form_equals_the_oracle(name, frames, ego, opt):
    """ every case, and the margins that let the GPU test ask for equality where cos / sin take part in a decision ('bev', '3d'): no value
    within 1e-9 of the threshold; on the drive no two candidates of a frame within 1e-9 of each other and, for 'optimal', section
    4.32's gap above 0.  (The carried crossing holds equal candidates by symmetry: they never compete for a slot or a row.) """
    values, matrices = [], []
    got = same_as_oracle(frames, ego, opt, values=values, matrices=matrices)
    assert (got[1] >= 0).sum() >= 16 and np.abs(got[4]).max() > 0.0
    to_thr, apart = K.margins(values, opt)
    print(name, 'to the threshold', to_thr, 'between candidates', apart)
    assert to_thr > 1e-9
    if name.startswith('drive'):
        assert apart > 1e-9
        if opt.get('assign') == 'optimal':
            gaps = optimal_gaps(matrices)
            print(name, 'min(gap - 2 pairs) =', min(gaps))
            assert gaps and min(gaps) > 0


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric', T.KF_METRICS)
def test_any_cut_into_calls_gives_the_same_result(metric, assign):
    """ every cut of the drive into two calls, one into four and one into single frames, each call with its slice of the records: the
    state and the covariance carry everything """
    frames = K.DRIVE
    ego = K.ego_kinds(len(frames))['general']
    opt = K.options(metric, K.THRESHOLDS[metric], assign, smooth=True)
    whole = T.track_rows_np(frames, opt, ego=ego)
    N = len(frames)
    for cuts in [[0, c, N] for c in range(1, N)] + [[0, 1, 4, 9, N], list(range(N + 1))]:
        state, cov, parts = None, None, []
        for a, b in zip(cuts, cuts[1:]):
            r, i, h, state, cov = T.track_rows_np(frames[a:b], opt, state, ego=ego[a:b], cov=cov)
            parts.append((r, i, h))
        for k in range(3):
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes()
        assert state.tobytes() == whole[3].tobytes() and cov.tobytes() == whole[4].tobytes()


def test_identity_records_change_nothing():
    """ R = I, t = 0: every covariance word equals the one without records (1 * a + 0 * b is a) """
    for metric in T.KF_METRICS:
        opt = K.options(metric, K.THRESHOLDS[metric])
        want = T.track_rows_np(K.DRIVE, opt)
        got = T.track_rows_np(K.DRIVE, opt, ego=K.ego_kinds(len(K.DRIVE))['identity'])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4]) and np.array_equal(got[3]['box'], want[3]['box'])


def test_list_input_the_empty_call_and_the_helpers():
    opt = K.options('maha')
    whole = T.track_rows_np(K.DRIVE, opt)
    as_list = T.track_rows_np(list(K.DRIVE), opt)
    assert isinstance(as_list[1], list) and as_list[3].tobytes() == whole[3].tobytes() and as_list[4].tobytes() == whole[4].tobytes()
    empty = T.track_rows_np(np.zeros((0, 8, 36), np.float32), opt, whole[3], cov=whole[4])
    assert len(empty) == 5 and empty[3].tobytes() == whole[3].tobytes() and empty[4].tobytes() == whole[4].tobytes()
    assert T.empty_cov().shape == (10, 128) and T.empty_cov(3).shape == (3, 10, 128) and not T.empty_cov(2).any()
    assert T.read_cov(whole[4].tobytes()).tobytes() == whole[4].tobytes() and T.read_cov(whole[4].tobytes()).shape == (10, 128)
    assert T.read_cov(np.stack([whole[4], whole[4]]).view(np.uint8).reshape(2, -1)).shape == (2, 10, 128)
    with pytest.raises(ValueError, match='no multiple'):
        T.read_cov(bytes(100))
    with pytest.raises(ValueError, match="no 'filter'"):
        T.track_rows_np(K.DRIVE, K.plain(K.options('dist')), cov=whole[4])
    assert len(T.track_rows_np(K.DRIVE, K.plain(K.options('dist')))) == 4         # without the filter: what it was
    # free slots hold zeros, occupied ones a covariance
    occupied = whole[3]['id1'] != 0
    assert not whole[4][:, ~occupied].any() and (whole[4][[AXX, AZZ, CXX, CZZ]][:, occupied] > 0.0).all()


# ---------------------------------------------------------------------------------------------------- what it is for
def test_no_fixed_threshold_tracks_the_demonstration_scene_and_the_filter_does():
    """ the issue's scene, exactly: every 'dist' threshold breaks F into more than one id or gives Q the id of P; 'maha' at 3 standard
    deviations gives the true three identities, with wide margins: F's m stays <= 2, P-to-Q is >= 30 against the gate's 9 """
    frames, gts = K.demo()
    for thr in K.DEMO_DIST:
        ids = T.track_rows_np(frames, O.options('dist', thr))[1]
        f_ids, inherits = len(set(ids[:, 0].tolist())), ids[5, 1] == ids[6, 1]
        print('dist', thr, 'ids of F', f_ids, 'Q inherits P', bool(inherits))
        assert f_ids > 1 or inherits
        assert (f_ids, bool(inherits)) == ((2, False) if thr < 4.5 else (2, True) if thr < 8.0 else (1, True))   # the issue's table
    for assign in T.ASSIGNS:
        opt = K.options('maha', assign=assign)
        values = []
        got = same_as_oracle(frames, None, opt, values=values)
        ids = got[1]
        assert ids[:, 0].tolist() == [0] * 12 and ids[:, 1].tolist() == [1] * 6 + [2] * 6 and int(got[3]['next_id']) == 3
        assert T.id_switches(gts, ids) == 0
        assert got[3]['id1'][:3].tolist() == [1, 0, 3]                             # F in slot 0, P was in slot 1 and has died, Q in slot 2
        f_m = [v for frame in values for v, t, d in frame if t == 0 and d == 0]
        p_q = [v for f, frame in enumerate(values) for v, t, d in frame if t == 1 and d == 1 and f >= 6]
        print(assign, 'F m max', max(f_m), 'P-to-Q m min', min(p_q))
        assert len(f_m) == 11 and max(f_m) <= 2.0
        assert len(p_q) == 3 and min(p_q) >= 30.0                                 # (P lives max_age = 2 frames beyond its last row)


def test_a_car_born_moving_is_caught_sooner():
    """ 1 m per frame, exact rows, born at v = 0: the position error behind the update of frames 1 - 4.  Recorded on the CPU:
    fixed gains (0.5, 0.25) 0.5 0.625 0.53125 0.3515625 m; Kalman (the demonstration's noise) 0.2021 0.1496 0.1028 0.0738 m """
    frames = K.mover()
    errors = {}
    for name, opt in (('fixed', O.options('dist', 2.3)), ('kalman', K.options('maha'))):
        state, cov, errors[name] = None, None, []
        for f in range(5):
            res = T.track_rows_np(frames[f:f + 1], opt, state, **({'cov': cov} if name == 'kalman' else {}))
            state, cov = res[3], res[4] if name == 'kalman' else None
            assert res[1][0, 0] == 0 and int(state['next_id']) == 1
            errors[name].append(float(np.hypot(state['box'][0][0] - 0.5, state['box'][2][0] - (20.0 + f))))
    print('fixed', errors['fixed'], 'kalman', errors['kalman'])
    assert errors['fixed'][0] == errors['kalman'][0] == 0.0
    for f in range(1, 5):
        assert errors['kalman'][f] < errors['fixed'][f], f


def test_200_matched_updates_keep_the_covariance_positive():
    """ one car, 200 frames (the issue states the length), every frame a matched update: the ten words are the upper triangle -- there
    is no second copy of an off-diagonal word that could drift --, A keeps det > 0, and so do the variances and the whole matrix """
    assert len(T.COV_FIELDS) == 10 == hip.GPP_TRACK_COV_FIELDS
    frames = K.steady(200)
    opt = K.options('maha')
    state, cov = None, None
    for f in range(len(frames)):
        _, ids, hits, state, cov = T.track_rows_np(frames[f:f + 1], opt, state, cov=cov)
        assert ids[0, 0] == 0 and hits[0, 0] == f + 1
        p = cov[:, 0]
        assert p[AXX] * p[AZZ] - p[AXZ] * p[AXZ] > 0.0 and p[AXX] > 0.0 and p[CXX] > 0.0 and p[CZZ] > 0.0
        full = np.array([[p[AXX], p[AXZ], p[BXX], p[BXZ]], [p[AXZ], p[AZZ], p[BZX], p[BZZ]],
                         [p[BXX], p[BZX], p[CXX], p[CXZ]], [p[BXZ], p[BZZ], p[CXZ], p[CZZ]]])
        assert np.linalg.eigvalsh(full).min() > 0.0
    want = K.track(frames[:40], opt)
    got = T.track_rows_np(frames[:40], opt)
    assert K.same_cov(want[4], got[4]) and O.same_state(want[3], got[3])


def test_a_quarter_turn_swaps_axx_and_azz_bit_for_bit():
    """ a frame without rows behind the drive, once with the identity record and once with a quarter turn about Y: A and C swap their
    diagonals and flip the sign of the off-diagonal word, bit for bit; B's words go where the turn sends them """
    opt = K.options('maha')
    _, _, _, state, cov = T.track_rows_np(K.DRIVE, opt)
    blank = padding_frame()
    same = T.track_rows_np(blank, opt, state, ego=np.array([E.IDENTITY]), cov=cov)[4]
    for turn, sign in ((E.LEFT, 1.0), (E.RIGHT, -1.0)):
        rec = np.array([E.record(turn, [0.0, 0.0, 0.0], sign * E.QUARTER)])
        got = T.track_rows_np(blank, opt, state, ego=rec, cov=cov)[4]
        want = K.track(blank, opt, rec, state_for_oracle(state), cov.tolist())[4]
        assert K.same_cov(want, got)
        occupied = state['id1'] != 0
        assert occupied.sum() == 6 and (same[AXX, occupied] != same[AZZ, occupied]).all()
        for a, b in ((AXX, AZZ), (AZZ, AXX), (CXX, CZZ), (CZZ, CXX), (BXX, BZZ), (BZZ, BXX)):
            assert got[a].tobytes() == same[b].tobytes()
        for k in (AXZ, CXZ):
            assert np.array_equal(got[k], -same[k])
        assert np.array_equal(got[BXZ], -same[BZX]) and np.array_equal(got[BZX], -same[BXZ])


def padding_frame(D=8):
    return O.padding(D)[None]


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric', T.KF_METRICS)
def test_a_covariance_that_is_not_positive_definite_takes_the_fallback(metric, assign):
    """ a caller's covariance with a negative Axx in slot 0: under 'bev' / '3d' / 'dist' the pair is matched by its metric, det is not
    > 0, the update is the fixed gains' and the covariance is set as at a birth from the matched row -- in the oracle and in the NumPy
    form alike (the kernel: tests/test_track_kf_gpu.py); under 'maha' such a slot has no candidate at all and a new track is born """
    state, cov, frames, opt = fallback_scene(metric, assign)
    branches = []
    got = same_as_oracle(frames, None, opt, state, cov, branches=branches)
    if metric == 'maha':
        assert branches == ['kalman'] and got[1][0].tolist() == [2, 1] and int(got[3]['misses'][0]) == 1
        return
    assert sorted(branches) == ['fallback', 'kalman'] and got[1][0].tolist() == [0, 1]
    fixed = T.track_rows_np(frames, K.plain(opt), state)[3]
    assert np.array_equal(got[3]['box'][:, 0], fixed['box'][:, 0])                # slot 0: the fixed gains' numbers
    assert not np.array_equal(got[3]['box'][:, 1], fixed['box'][:, 1])            # slot 1: the Kalman update
    noise = T.row_noise(frames[0], opt['noise'])[:, 0]
    assert got[4][:, 0].tolist() == noise.tolist() + [0.0] * 4 + [4.0, 0.0, 4.0]


def fallback_scene(metric, assign):
    opt = K.options(metric, K.THRESHOLDS[metric], assign)
    first = O.frames_of([[O.row(0.9, -3.0, 20.0), O.row(0.8, 4.0, 30.0)]], 2)
    _, _, _, state, cov = T.track_rows_np(first, opt)
    cov = cov.copy()
    cov[AXX, 0] = -64.0
    frames = O.frames_of([[O.row(0.9, -2.875, 20.25), O.row(0.8, 4.125, 29.75)]], 2)
    return state, cov, frames, opt


CROWDS = [('maha', 'optimal', True), ('maha', 'greedy', False), ('dist', 'optimal', True), ('dist', 'greedy', False)]


def crowd(metric, assign, records):
    """ tests/track_crowd_cases.py's lattice of 128 x 128 cars that all overlap, its first two frames: 128 births, then 128 slots against
    128 rows; behind quarter and half turns (records) or from a still camera -> (frames, ego or None, options) """
    import track_crowd_cases as C
    if records:
        frames, ego = C.carried('lattice_128x128', E.TURNS)
        ego = ego[:2]
    else:
        frames, ego = C.scenes()['lattice_128x128'], None
    return frames[:2], ego, K.options(metric, {'maha': K.GATE, 'dist': 2.3}[metric], assign, smooth=True)


@pytest.mark.parametrize('metric,assign,records', CROWDS)
def test_one_crowded_frame(metric, assign, records):
    """ the scene of the GPU test: every slot finds a row again, and under 'maha' every one of the 16 384 pairs is inside the gate """
    frames, ego, opt = crowd(metric, assign, records)
    keys = []
    T.track_rows_np(frames, opt, ego=ego, keys_out=keys)
    got = same_as_oracle(frames, ego, opt)
    assert (got[2][1] == 2).sum() == 128 and int(got[3]['next_id']) == 128 and (got[4][0] > 0.0).all()
    assert np.isfinite(keys[1]).sum() == (16384 if metric == 'maha' else 12808)


# ---------------------------------------------------------------------------------------------------- the option
def test_check_option_takes_the_filter():
    base = {'metric': 'maha', 'threshold': 3.0}
    opt = T.check_option(dict(base, filter='kalman', noise=K.NOISE))
    assert opt == dict(T.DEFAULTS, filter='kalman', noise=K.NOISE, **base) and T.check_option(opt) == opt
    lists = {'radial': [0.1, 0.05], 'tangential': [0.1, 0.005], 'process': [0.01, 0.01], 'birth_speed': 2}
    assert T.check_option(dict(base, filter='kalman', noise=lists)) == opt
    for metric, thr in (('dist', 2.0), ('bev', 0.25), ('3d', 0.0)):                  # the other metrics stay available with the filter
        assert T.check_option({'metric': metric, 'threshold': thr, 'filter': 'kalman', 'noise': K.NOISE})['filter'] == 'kalman'
    both = T.check_option(dict(base, filter='kalman', noise=K.NOISE, assign='optimal', ego=True))
    assert both['assign'] == 'optimal' and both['ego'] is True and T.is_optimal(both)
    fixed = T.check_option({'metric': 'dist', 'threshold': 2.0, 'filter': 'fixed'})
    assert fixed == dict(T.DEFAULTS, metric='dist', threshold=2.0) and 'filter' not in fixed and T.kf_params_of(fixed) is None
    assert T.METRICS == ('bev', '3d', 'dist') and T.KF_METRICS == T.METRICS + ('maha',)
    kf = T.kf_params_of(opt)
    assert [getattr(kf, n) for n, _ in hip.TrackKfParams._fields_] == [0.1, 0.05, 0.1, 0.005, 0.01, 0.01, 2.0, 0]
    assert T.params_of(opt).metric == 3 and T.params_of(opt).threshold == 3.0


def bad_noise():
    nan, inf = float('nan'), float('inf')
    out = [dict(K.NOISE, radial=(0.0, 0.05)), dict(K.NOISE, radial=(-0.1, 0.05)), dict(K.NOISE, radial=(0.1, -0.05)), dict(K.NOISE, radial=(nan, 0.05)),
           dict(K.NOISE, radial=(0.1, inf)), dict(K.NOISE, radial=0.1), dict(K.NOISE, radial=(0.1, 0.05, 0.0)), dict(K.NOISE, tangential=(0.0, 0.0)),
           dict(K.NOISE, tangential=(0.1, nan)), dict(K.NOISE, process=(-0.01, 0.01)), dict(K.NOISE, process=(0.01, inf)),
           dict(K.NOISE, process=(0.01,)), dict(K.NOISE, birth_speed=0.0), dict(K.NOISE, birth_speed=-2.0), dict(K.NOISE, birth_speed=nan),
           dict(K.NOISE, birth_speed=inf), dict(K.NOISE, birth_speed='fast'), dict(K.NOISE, more=1), {}, None, (0.1, 0.05)]
    out.append({k: v for k, v in K.NOISE.items() if k != 'process'})
    return out


@pytest.mark.parametrize('noise', bad_noise(), ids=[str(k) for k in range(len(bad_noise()))])
def test_check_option_refuses_bad_noise(noise):
    with pytest.raises(ValueError, match='noise|radial|process|birth_speed'):
        T.check_option({'metric': 'maha', 'threshold': 3.0, 'filter': 'kalman', 'noise': noise})


def test_check_option_refuses_the_metric_without_the_filter_and_the_rest():
    with pytest.raises(ValueError, match="needs 'filter': 'kalman'"):
        T.check_option(('maha', 3.0))
    with pytest.raises(ValueError, match="needs 'filter': 'kalman'"):
        T.check_option({'metric': 'maha', 'threshold': 3.0, 'filter': 'fixed'})
    with pytest.raises(ValueError, match='no defaults'):
        T.check_option({'metric': 'maha', 'threshold': 3.0, 'filter': 'kalman'})
    with pytest.raises(ValueError, match="needs 'filter': 'kalman'"):
        T.check_option({'metric': 'dist', 'threshold': 2.0, 'noise': K.NOISE})
    for kind in ('ekf', None, 1, True):
        with pytest.raises(ValueError, match='filter'):
            T.check_option({'metric': 'dist', 'threshold': 2.0, 'filter': kind, 'noise': K.NOISE})
    for thr in (0.0, -3.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='maha threshold'):
            T.check_option({'metric': 'maha', 'threshold': thr, 'filter': 'kalman', 'noise': K.NOISE})
    with pytest.raises(ValueError):
        T.metric_code('maha')
    assert T.metric_code('maha', True) == 3 and T.metric_code('dist', True) == 2 == T.metric_code('dist')


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_constants_and_contract():
    text = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    define = lambda name: int(re.search(r'#define {}\s+(\d+)'.format(name), text).group(1))  # noqa: E731
    assert define('GPP_TRACK_MAHA') == 3 == hip.GPP_TRACK_MAHA == T.KF_METRICS.index('maha')
    assert define('GPP_TRACK_COV_FIELDS') == 10 == hip.GPP_TRACK_COV_FIELDS == len(T.COV_FIELDS)
    assert ctypes.sizeof(hip.TrackKfParams) == 64 and ctypes.sizeof(hip.TrackState) == 12304      # gpp_track_state keeps its bytes
    struct = text[text.index('typedef struct gpp_track_kf_params'):text.index('} gpp_track_kf_params;')]
    names = re.findall(r'(\w+)\s*[;,]', re.sub(r'/\*.*?\*/', '', struct))
    assert names == [n for n, _ in hip.TrackKfParams._fields_]
    contract = text[text.index('Tracking with a KALMAN FILTER'):text.index('#define GPP_TRACK_MAHA')]
    contract = ' '.join(re.sub(r'\n \*', ' ', contract).split())
    for phrase in ('A += B + B^T + C + q_pos I', 'B += C', 'C += q_vel I', 'Rg = [[R00, R02], [R20, R22]]', 'det > 0 and m < threshold * threshold',
                   'K = [A; B^T] S^-1', 'A = R of the row, B = 0, C = birth_speed^2 I', 'cov_out == cov_in is allowed', 'or null: no records',
                   'go on refusing GPP_TRACK_MAHA', 'cov_in to cov_out', "What pitch and roll mix in from y is left out"):
        assert phrase in contract, phrase
    n = ctypes.c_size_t(0)
    assert hip.lib().gpp_track_cov_bytes(ctypes.byref(n)) == 0 and n.value == 10240 == hip.track_cov_bytes() == T.empty_cov().nbytes
    assert hip.lib().gpp_track_cov_bytes(None) == -1


GOOD_KF = dict(radial0=0.1, radial1=0.05, tangential0=0.1, tangential1=0.005, q_pos=0.01, q_vel=0.01, birth_speed=2.0, reserved=0)


def kf_call(kf=None, params=None, ego=None, assign=0, N=4, D=129, seq=(0, 4), null_kf=False):
    """ host code: every device pointer is null -- a refusal returns before it is looked at.  With D = 129 a call that passes every
    argument check is GPP_ERR_UNSUPPORTED (-4), which comes behind them: -1 then means the argument """
    p = hip.TrackParams(3, 2, 0, 0, 3.0, 0.5, 0.25, 0.25, 0.0) if params is None else params
    k = hip.TrackKfParams(**dict(GOOD_KF, **(kf or {})))
    seq = (ctypes.c_int32 * len(seq))(*seq)
    e = None if ego is None else np.ascontiguousarray(ego, np.float64).ctypes.data_as(ctypes.c_void_p)
    return hip.lib().gpp_track_kf_f64(None, N, D, seq, len(seq) - 1, None, None, None, None, ctypes.byref(p), None if null_kf else ctypes.byref(k),
                                      e, assign, None, None, None, None, 0, None)


def test_c_abi_refuses_before_any_launch():
    nan, inf = float('nan'), float('inf')
    records = np.array([E.IDENTITY] * 4)
    assert kf_call() == -4 and kf_call(ego=records) == -4 and kf_call(assign=1) == -4     # a null `ego` is no error here
    assert kf_call(D=4, seq=(0,)) == 0 and kf_call(N=0, D=4, seq=(0,)) == 0               # S == 0: GPP_OK
    assert kf_call(null_kf=True) == -1
    for name in ('radial0', 'tangential0', 'birth_speed'):
        for value in (0.0, -0.5, nan, inf, -inf):
            assert kf_call({name: value}) == -1, (name, value)
    for name in ('radial1', 'tangential1', 'q_pos', 'q_vel'):
        assert kf_call({name: 0.0}) == -4
        for value in (-1e-300, nan, inf, -inf):
            assert kf_call({name: value}) == -1, (name, value)
    for word in (1, -1, 1 << 40):
        assert kf_call({'reserved': word}) == -1
    for assign in (-1, 2):
        assert kf_call(assign=assign) == -1
    # the threshold of the fourth metric is in standard deviations: finite and > 0; the others keep their rules under the filter
    for thr in (0.0, -1.0, nan, inf):
        assert kf_call(params=hip.TrackParams(3, 2, 0, 0, thr, 0.5, 0.25, 0.25, 0.0)) == -1
    assert kf_call(params=hip.TrackParams(3, 2, 0, 0, 1.5, 0.5, 0.25, 0.25, 0.0)) == -4       # (1.5 is no overlap, but a fine gate)
    assert kf_call(params=hip.TrackParams(0, 2, 0, 0, 1.5, 0.5, 0.25, 0.25, 0.0)) == -1
    assert kf_call(params=hip.TrackParams(2, 2, 0, 0, 2.0, 0.5, 0.25, 0.25, 0.0)) == -4
    assert kf_call(params=hip.TrackParams(4, 2, 0, 0, 2.0, 0.5, 0.25, 0.25, 0.0)) == -1
    assert kf_call(params=hip.TrackParams(3, 2, 0, 1, 3.0, 0.5, 0.25, 0.25, 0.0)) == -1       # gpp_track_f64's own
    bad = records.copy()
    bad[2, 0] = nan
    assert kf_call(ego=bad) == -1 and kf_call(ego=bad, seq=(0, 2)) == -4                  # gpp_track_ego_f64's own
    assert kf_call(D=4) == -1 and kf_call(N=0, D=4, seq=(0, 0)) == -1                     # S > 0 and null states / covariances
    # the three entry points without the filter go on refusing metric code 3
    maha = hip.TrackParams(3, 2, 0, 0, 3.0, 0.5, 0.25, 0.25, 0.0)
    seq = (ctypes.c_int32 * 2)(0, 4)
    lib = hip.lib()
    assert lib.gpp_track_f64(None, 4, 129, seq, 1, None, None, ctypes.byref(maha), None, None, None, None, 0, None) == -1
    assert lib.gpp_track_optimal_f64(None, 4, 129, seq, 1, None, None, ctypes.byref(maha), None, None, None, None, 0, None) == -1
    assert lib.gpp_track_ego_f64(None, 4, 129, seq, 1, None, None, ctypes.byref(maha), records.ctypes.data_as(ctypes.c_void_p), 0,
                                 None, None, None, None, 0, None) == -1


# ---------------------------------------------------------------------------------------------------- the command lines
KALMAN_ARGS = ['--track-filter', 'kalman', '--track-noise', '0.1', '0.05', '0.1', '0.005', '--track-process', '0.01', '0.01', '--track-birth-speed', '2']


def write_results(directory, frames):
    """ the demonstration scene as KITTI result files, one per frame """
    from keras_retinanet_3D.utils import gpp_utils
    os.mkdir(directory)
    for k, rows in enumerate(frames):
        with open(os.path.join(directory, '%06d.txt' % k), 'w') as f:
            f.write(gpp_utils.kitti_lines_from_rows(rows, int((rows[:, 14] >= 0).sum())))


def test_track_results_host_writes_the_host_forms_tracks(tmp_path):
    """ bin/track_results.py --host --metric maha --track-filter kalman ... on result files: the lines of tracking_lines over
    track_rows_np of the rows it read; three identities on the demonstration scene, which no --metric dist threshold gives """
    from keras_retinanet_3D.bin import track_results
    write_results(str(tmp_path / 'kitti'), K.demo()[0])
    common = [str(tmp_path / 'kitti'), str(tmp_path / 'tracks.txt')]
    track_results.main(common + ['--metric', 'maha', '--threshold', '3', '--host'] + KALMAN_ARGS)
    names, frames = track_results.read_sequence(str(tmp_path / 'kitti'))
    _, ids, hits, state, _ = T.track_rows_np(frames, K.options('maha'))
    assert (tmp_path / 'tracks.txt').read_text() == ''.join(T.tracking_lines(k, frames[k], ids[k], hits[k]) for k in range(12))
    assert int(state['next_id']) == 3 and sorted({int(line.split()[1]) for line in (tmp_path / 'tracks.txt').read_text().splitlines()}) == [0, 1, 2]
    track_results.main(common + ['--track', 'dist', '--threshold', '8', '--host'])          # (--track is --metric's other name here)
    assert sorted({int(line.split()[1]) for line in (tmp_path / 'tracks.txt').read_text().splitlines()}) == [0, 1]
    for bad in (['--metric', 'maha', '--threshold', '3'], ['--metric', 'maha', '--threshold', '3', '--track-filter', 'kalman'],
                ['--metric', 'dist', '--threshold', '3', '--track-birth-speed', '2'],
                ['--metric', 'maha', '--threshold', '3'] + KALMAN_ARGS[:-1] + ['0'], ['--metric', 'bev', '--threshold', '3'] + KALMAN_ARGS):
        with pytest.raises(SystemExit):
            track_results.parse_args(common + bad)
    assert track_results.parse_args(common + ['--metric', 'bev', '--threshold', '0.3'] + KALMAN_ARGS).option['filter'] == 'kalman'


def test_run_network_takes_the_filter():
    from keras_retinanet_3D.bin import run_network
    common = ['synthetic:1234.h5', 'img', 'calib', 'planes', 'out', '--kitti', '--device-pose']
    args = run_network.parse_args(common + ['--track', 'maha', '--track-threshold', '3', '--track-assign', 'optimal'] + KALMAN_ARGS)
    assert run_network.track_option(args) == {'metric': 'maha', 'threshold': 3.0, 'max_age': 2, 'smooth': False, 'assign': 'optimal',
                                              'filter': 'kalman', 'noise': K.NOISE}
    plain = run_network.parse_args(common + ['--track', 'dist', '--track-threshold', '3'])
    assert run_network.track_option(plain) == {'metric': 'dist', 'threshold': 3.0, 'max_age': 2, 'smooth': False}
    for bad in (['--track', 'maha', '--track-threshold', '3'], ['--track', 'maha', '--track-threshold', '3', '--track-filter', 'kalman'],
                ['--track', 'dist', '--track-threshold', '3', '--track-noise', '0.1', '0.05', '0.1', '0.005'], KALMAN_ARGS,
                ['--track', 'maha', '--track-threshold', '0'] + KALMAN_ARGS):
        with pytest.raises(SystemExit):
            run_network.parse_args(common + bad)
