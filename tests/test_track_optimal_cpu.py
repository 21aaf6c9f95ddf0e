""" CPU tests of the tracker's optimal assignment: the NumPy form (utils/track.py, 'assign': 'optimal') against
the loop-written oracle (tests/track_optimal_oracle.py); every frame's total against scipy's; the two scenes in which the assignment
matters, with their numbers; the margins that let tests/test_track_optimal_gpu.py ask for equality; the option and the command lines; the
C ABI's argument checks (host code: they come before any launch). """
import ctypes
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import track_optimal_oracle as P
import track_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import mot_eval
from keras_retinanet_3D.utils import track as T

EXACT = P.exact_cases()
MARGIN = P.margin_cases()
ids_of = lambda cases: [c[0] for c in cases]  # noqa: E731
# min over the frames of (second-best total - best total - 2 matched pairs), measured with the finished NumPy form
MEASURED_GAPS = {'drive_dist': 881911, 'drive_bev': 497958, 'drive_3d': 448549, 'dense_drive_dist': 237781}


def same_as_oracle(frames, opt):
    matrices = []
    want_rows, want_ids, want_hits, want_state = P.track(frames, opt, matrices=matrices)
    got_rows, got_ids, got_hits, got_state = T.track_rows_np(frames, opt)
    assert got_rows.dtype == np.float32 and got_ids.dtype == np.int32 and got_hits.dtype == np.int32
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_hits, want_hits)
    assert O.same_state(want_state, got_state)
    cols = [c for c in range(36) if c != 25 or not opt['smooth']]
    assert np.array_equal(got_rows[..., cols].view(np.uint32), want_rows[..., cols].view(np.uint32))       # bit for bit, NaN included
    close = np.abs(got_rows[..., 25].astype(np.float64) - want_rows[..., 25]) <= 4 * np.spacing(np.abs(want_rows[..., 25]))
    assert (close | (got_rows[..., 25].view(np.uint32) == want_rows[..., 25].view(np.uint32))).all()
    return matrices


def host_matrices(frames, opt):
    """ per frame (cost, slots, rows, pairs) of the NumPy form: cost_cells and optimal over the table step_np built """
    opt = T.check_option(opt)
    state, out = T.empty_state(), []
    for rows in np.asarray(frames, np.float32):
        occupied = state['id1'] != 0
        valid = (rows[:, 14] >= 0.0) & ~np.isnan(rows[:, T.ROW_COLS]).any(axis=1)
        keys = []
        T.step_np(state, rows, opt, keys)
        cost, ts, ds = T.cost_cells(keys[0], occupied, valid, opt['metric'], opt['threshold'])
        out.append((cost, ts, ds, T.optimal(keys[0], occupied, valid, opt['metric'], opt['threshold'])))
    return out


def total_of(cost):
    """ scipy's minimum total of a square integer matrix (exact: the sums stay far below 2^53) """
    cost = np.asarray(cost, np.int64).reshape(len(cost), len(cost))
    r, c = linear_sum_assignment(cost)
    return int(cost[r, c].sum())


def check_totals(frames, opt, oracle_matrices):
    """ on every frame: the oracle's matrix == cost_cells', both assignments reach scipy's total, and the pairs are the same """
    host = host_matrices(frames, opt)
    assert len(host) == len(oracle_matrices) == len(frames)
    for (cost, ts, ds, pairs), (o_cost, o_slots, o_rows, o_pairs) in zip(host, oracle_matrices):
        n = max(len(ts), len(ds))
        assert cost.shape == (n, n) and cost.dtype == np.int32 and cost.tolist() == o_cost
        assert ts.tolist() == o_slots and ds.tolist() == o_rows and sorted(pairs) == o_pairs
        best = total_of(cost)
        col, total = mot_eval.assign_np(cost)
        assert total == best and sorted(col.tolist()) == list(range(n))
        p = P.assign(o_cost)
        assert sum(o_cost[p[j]][j] for j in range(n)) == best
        assert all(0 <= cost[i, j] < T.SCALE for i, j in [(list(ts).index(t), list(ds).index(d)) for t, d in pairs])
    return host


@pytest.mark.parametrize('name,frames,opt', EXACT, ids=ids_of(EXACT))
def test_host_form_equals_the_oracle_on_the_exact_cases(name, frames, opt):
    values = []
    P.track(frames, opt, values=values)
    to_thr, _ = O.margins(values, opt)
    assert to_thr > 1e-9, to_thr                       # (no candidate sits on the threshold; equal candidates are wanted here)
    check_totals(frames, opt, same_as_oracle(frames, opt))


def second_best_gap(cost, ts, ds, pairs):
    """ (the smallest total with one matched candidate forbidden) - (the best total) - 2 * (matched pairs); None without a pair """
    if not pairs:
        return None
    best, second = total_of(cost), None
    for t, d in pairs:
        forbidden = cost.copy()
        forbidden[list(ts).index(t), list(ds).index(d)] = T.SCALE
        total = total_of(forbidden)
        second = total if second is None else min(second, total)
    return second - best - 2 * len(pairs)


@pytest.mark.parametrize('name,frames,opt', MARGIN, ids=ids_of(MARGIN))
def test_host_form_equals_the_oracle_where_the_margins_hold(name, frames, opt):
    """ what lets the GPU test ask for equality.  Candidacy: no value within 1e-9 of the threshold (section 4.28's margin).  The
    assignment: a last-bit difference in a key moves a cell by at most 1, so a total by at most the number of matched pairs; the best
    total is therefore alone as long as the second-best total lies more than 2 * (matched pairs) above it """
    values = []
    P.track(frames, opt, values=values)
    to_thr, _ = O.margins(values, opt)
    assert to_thr > 1e-9, to_thr
    host = check_totals(frames, opt, same_as_oracle(frames, opt))
    gaps = [g for g in (second_best_gap(*h) for h in host) if g is not None]
    print(name, 'min(gap - 2 pairs) =', min(gaps))
    assert gaps and min(gaps) > 0
    if name in MEASURED_GAPS:
        assert min(gaps) == MEASURED_GAPS[name], (name, min(gaps))


def test_the_steal():
    """ the two-by-two case: greedy gives track 0 the nearer row, track 1 misses and a third id is born; the optimum pairs both """
    frames = P.steal()
    _, ids, hits, state = T.track_rows_np(frames, P.optimal(P.STEAL_OPTION))
    assert ids.tolist() == [[0, 1], [1, 0]] and hits[1].tolist() == [2, 2] and int(state['next_id']) == 2
    _, greedy_ids, _, greedy_state = T.track_rows_np(frames, P.STEAL_OPTION)
    assert greedy_ids.tolist() == [[0, 1], [0, 2]] and int(greedy_state['next_id']) == 3 and int(greedy_state['misses'][1]) == 1
    cost, ts, ds, pairs = host_matrices(frames, P.optimal(P.STEAL_OPTION))[1]
    assert cost.tolist() == [[200704, 262144], [331776, 1 << 20]] and ts.tolist() == [0, 1] and ds.tolist() == [0, 1]
    assert pairs == [(0, 1), (1, 0)] and mot_eval.assign_np(cost)[1] == 593920 == total_of(cost)
    # greedy's own pairs cost more: the near pair and one miss
    assert cost[0, 0] + cost[1, 1] == 200704 + (1 << 20) > 593920


def test_the_dense_drive():
    """ ten cars in lanes 1.75 m apart, 0.4 m of noise, threshold 2.3 m: greedy 3 switches and 11 ids, the optimum none and 10 """
    frames, gts = P.dense_drive(with_gt=True)
    _, ids, _, state = T.track_rows_np(frames, O.options('dist'))
    assert T.id_switches(gts, ids) == 3 and int(state['next_id']) == 11
    _, ids, _, state = T.track_rows_np(frames, P.optimal(O.options('dist')))
    assert T.id_switches(gts, ids) == 0 and int(state['next_id']) == 10 and sorted(set(ids[ids >= 0].tolist())) == list(range(10))


def test_nothing_changes_where_greedy_is_right():
    """ tests/track_oracle.drive as the suite uses it (6 m lanes): the same ids, hits and state bytes under either assignment """
    for metric in T.METRICS:
        frames = O.drive(O.DRIVE_SEED)
        greedy, best = T.track_rows_np(frames, O.options(metric)), T.track_rows_np(frames, P.optimal(O.options(metric)))
        assert np.array_equal(greedy[1], best[1]) and np.array_equal(greedy[2], best[2]) and greedy[3].tobytes() == best[3].tobytes()


def test_cells():
    """ the cells' edges: a candidate's cell lies in [0, 2^20 - 1] whatever its value, everything else is 2^20 """
    keys = np.full((T.MAX_TRACKS, 3), np.inf)
    occupied, valid = np.zeros(T.MAX_TRACKS, bool), np.array([True, False, True])
    occupied[[2, 5]] = True
    keys[2, 0], keys[5, 2] = 0.0, np.nextafter(4.0, 0.0)             # q = 0 and the largest q below threshold^2
    cost, ts, ds = T.cost_cells(keys, occupied, valid, 'dist', 2.0)
    assert ts.tolist() == [2, 5] and ds.tolist() == [0, 2] and cost.tolist() == [[0, 1 << 20], [1 << 20, (1 << 20) - 1]]
    assert P.cell(0.0, 'dist', 2.0) == 0 and P.cell(float(np.nextafter(4.0, 0.0)), 'dist', 2.0) == (1 << 20) - 1
    keys[2, 0], keys[5, 2] = -1.0, -1e-9                             # overlap 1 and an overlap below 2^-20
    cost, _, _ = T.cost_cells(keys, occupied, valid, 'bev', 0.0)
    assert cost.tolist() == [[0, 1 << 20], [1 << 20, (1 << 20) - 1]]
    assert P.cell(1.0, 'bev', 0.0) == 0 and P.cell(1e-9, 'bev', 0.0) == (1 << 20) - 1 and P.cell(0.5, '3d', 0.0) == 1 << 19
    occupied[:] = False                                               # rows but no slots: three padding rows
    cost, ts, ds = T.cost_cells(keys, occupied, valid, 'bev', 0.0)
    assert cost.shape == (2, 2) and (cost == T.SCALE).all() and ts.size == 0 and T.optimal(keys, occupied, valid, 'bev', 0.0) == []
    cost, _, _ = T.cost_cells(keys, occupied, np.zeros(3, bool), 'bev', 0.0)
    assert cost.shape == (0, 0)
    assert T.SCALE == 1 << 20 == P.S == mot_eval.SCALE


# ---------------------------------------------------------------------------------------------------- options and command lines
def test_check_option_takes_assign():
    base = {'metric': 'dist', 'threshold': 2.0}
    assert T.check_option(dict(base, assign='optimal')) == dict(T.DEFAULTS, assign='optimal', **base)
    assert T.check_option(dict(base, assign='greedy')) == dict(T.DEFAULTS, **base) and 'assign' not in T.check_option(dict(base, assign='greedy'))
    once = T.check_option(dict(base, assign='optimal'))
    assert T.check_option(once) == once and T.is_optimal(once) and not T.is_optimal(base) and not T.is_optimal(('bev', 0.1))
    for bad in ('hungarian', 'Optimal', '', None, 1, True):
        with pytest.raises(ValueError, match='assign'):
            T.check_option(dict(base, assign=bad))
    with pytest.raises(ValueError):
        T.check_option(dict(base, age=1))                              # an unknown key is still refused
    # the greedy round trips are what they were
    assert 'assign' not in T.DEFAULTS and T.check_option(('bev', 0)) == dict(T.DEFAULTS, metric='bev', threshold=0.0)
    full = {'metric': 'dist', 'threshold': 2.0, 'max_age': 0, 'gains': (1.0, 0.0, 1.0), 'birth_score': -1.0, 'smooth': True}
    assert T.check_option(full) == full and T.check_option(T.check_option(full)) == full
    assert T.ASSIGNS == ('greedy', 'optimal')


def test_model_refuses_an_unknown_assignment_before_the_device():
    from keras_retinanet_3D import models
    from keras_retinanet_3D.models import weights as W
    w = W.synthetic_weights('resnet50', 1)
    with pytest.raises(ValueError, match='needs pose=True'):
        models.load_model(w, backbone_name='resnet50', track={'metric': 'dist', 'threshold': 2.0, 'assign': 'optimal'})
    with pytest.raises(ValueError, match='assign'):
        models.load_model(w, backbone_name='resnet50', pose=True, track={'metric': 'dist', 'threshold': 2.0, 'assign': 'best'})


def test_command_line_arguments(tmp_path):
    from keras_retinanet_3D.bin import run_network, track_results
    base = ['m.h5', 'img', 'calib', 'planes.mat', 'out', '--device-pose', '--track', 'dist', '--track-threshold', '2']
    args = run_network.parse_args(base + ['--track-assign', 'optimal'])
    assert run_network.track_option(args) == {'metric': 'dist', 'threshold': 2.0, 'max_age': 2, 'smooth': False, 'assign': 'optimal'}
    four = {'metric': 'dist', 'threshold': 2.0, 'max_age': 2, 'smooth': False}
    assert run_network.track_option(run_network.parse_args(base)) == four
    assert run_network.track_option(run_network.parse_args(base + ['--track-assign', 'greedy'])) == four
    with pytest.raises(SystemExit):
        run_network.parse_args(base + ['--track-assign', 'hungarian'])
    common = ['dir', 'tracks.txt', '--metric', 'dist', '--threshold', '2']
    assert track_results.parse_args(common + ['--track-assign', 'optimal']).option['assign'] == 'optimal'
    assert 'assign' not in track_results.parse_args(common).option
    with pytest.raises(SystemExit):
        track_results.parse_args(common + ['--track-assign', 'hungarian'])
    # the host path of track_results.py on the steal: frame 1's rows keep the ids 1 and 0; greedy writes 0 and 2
    line = 'Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 {:.3f} 1.65 {:.2f} 0.00 {:.2f}\n'
    (tmp_path / 'r').mkdir()
    (tmp_path / 'r' / '000000.txt').write_text(line.format(0.0, 20.0, 0.9) + line.format(2.0, 20.0, 0.8))
    (tmp_path / 'r' / '000001.txt').write_text(line.format(0.875, 20.0, 0.9) + line.format(-1.0, 20.0, 0.8))
    run = [str(tmp_path / 'r'), str(tmp_path / 't.txt'), '--metric', 'dist', '--threshold', '2', '--host']
    track_results.main(run + ['--track-assign', 'optimal'])
    assert [ln.split()[:2] for ln in (tmp_path / 't.txt').read_text().splitlines()] == [['0', '0'], ['0', '1'], ['1', '1'], ['1', '0']]
    track_results.main(run)
    assert [ln.split()[:2] for ln in (tmp_path / 't.txt').read_text().splitlines()] == [['0', '0'], ['0', '1'], ['1', '0'], ['1', '2']]


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_contract():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'gpp.h')).read()
    contract = text[text.index('Tracking with an OPTIMAL one-to-one assignment'):text.index('int gpp_track_optimal_f64(')]
    contract = ' '.join(re.sub(r'\n \*', ' ', contract).split())                 # (the comment's line starts are no words)
    for phrase in ('n = max(T, R)', 'min(floor(x), S - 1)', 'min(S - k, S - 1)', 'every padding cell', 'NOT gpp_mot_assign\'s GPP_MOT_BIG form',
                   'ties to the first column', 'reserved != 0 is refused by both', 'gpp_track_workspace_bytes(S)', 'its cell is below S'):
        assert phrase in contract, phrase
    declared = lambda name: ' '.join(text[text.index('int {}('.format(name)):].split(';')[0].split()).replace(name, 'f')  # noqa: E731
    assert declared('gpp_track_optimal_f64') == declared('gpp_track_f64')                                     # one signature
    makefile = open(os.path.join(root, 'ground-plane-polling_amd', 'csrc', 'Makefile')).read()
    assert 'track.o: track.hip rot_iou.h mot_assign.h' in makefile


def bad_params():
    """ [(what, TrackParams, seq_start, D, code)] of include/gpp.h's error list: gpp_track_f64's, which gpp_track_optimal_f64 shares """
    good = dict(metric=2, max_age=2, smooth=0, reserved=0, threshold=2.0, gain_a=0.5, gain_b=0.25, gain_c=0.25, birth_score=0.0)
    nan, out = float('nan'), []
    for what, change in [('metric', dict(metric=3)), ('metric_negative', dict(metric=-1)), ('iou_thr_1', dict(metric=0, threshold=1.0)),
                         ('iou_thr_negative', dict(metric=1, threshold=-0.01)), ('iou_thr_nan', dict(metric=0, threshold=nan)),
                         ('dist_thr_0', dict(threshold=0.0)), ('dist_thr_inf', dict(threshold=float('inf'))), ('dist_thr_nan', dict(threshold=nan)),
                         ('a_0', dict(gain_a=0.0)), ('a_above', dict(gain_a=1.01)), ('a_nan', dict(gain_a=nan)), ('b_negative', dict(gain_b=-0.1)),
                         ('b_above', dict(gain_b=1.5)), ('b_nan', dict(gain_b=nan)), ('c_negative', dict(gain_c=-0.1)), ('c_above', dict(gain_c=2.0)),
                         ('c_nan', dict(gain_c=nan)), ('max_age', dict(max_age=-1)), ('birth_nan', dict(birth_score=nan)),
                         ('smooth', dict(smooth=2)), ('reserved', dict(reserved=1))]:
        out.append((what, hip.TrackParams(**dict(good, **change)), [0, 4], 4, -1))
    out += [('seq_descending', hip.TrackParams(**good), [3, 2], 4, -1), ('seq_beyond', hip.TrackParams(**good), [0, 5], 4, -1),
            ('seq_negative', hip.TrackParams(**good), [-1, 4], 4, -1), ('d_129', hip.TrackParams(**good), [0, 4], 129, -4)]
    return out


@pytest.mark.parametrize('what,params,seq,D,code', bad_params(), ids=[b[0] for b in bad_params()])
def test_c_abi_refuses_before_any_launch(what, params, seq, D, code):
    """ host code: every pointer is null -- a refusal returns before it is looked at """
    lib = hip.lib()
    seq = (ctypes.c_int32 * len(seq))(*seq)
    rc = lib.gpp_track_optimal_f64(None, 4, D, seq, len(seq) - 1, None, None, ctypes.byref(params), None, None, None, None, 0, None)
    assert rc == code


def test_c_abi_null_arguments_and_no_sequence():
    good = hip.TrackParams(2, 2, 0, 0, 2.0, 0.5, 0.25, 0.25, 0.0)
    seq = (ctypes.c_int32 * 2)(0, 4)
    call = hip.lib().gpp_track_optimal_f64
    assert call(None, 4, 4, None, 1, None, None, ctypes.byref(good), None, None, None, None, 0, None) == -1
    assert call(None, 4, 4, seq, 1, None, None, None, None, None, None, None, 0, None) == -1
    assert call(None, 4, 4, seq, 1, None, None, ctypes.byref(good), None, None, None, None, 0, None) == -1      # S > 0 without states
    assert call(None, 4, 4, seq, 0, None, None, ctypes.byref(good), None, None, None, None, 0, None) == 0       # S == 0
    assert call.argtypes == hip.lib().gpp_track_f64.argtypes
