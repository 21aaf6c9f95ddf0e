""" CPU tests of the tracker: the NumPy form (utils/track.py) against the loop-written oracle
(tests/track_oracle.py) on the issue's cases and on seeded scenes; the margins that let tests/test_track_gpu.py ask for equality; the
header's constants and contract; the option's argument errors; the C ABI's argument checks (host code: they come before any launch); the
tracking text; the identity switches. """
import ctypes
import math
import os
import re

import numpy as np
import pytest

import track_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import track as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = O.exact_cases()
MARGIN = O.margin_cases()
ids_of = lambda cases: [c[0] for c in cases]  # noqa: E731


def same_as_oracle(frames, opt, state=None, ostate=None):
    want_rows, want_ids, want_hits, want_state = O.track(frames, opt, ostate)
    got_rows, got_ids, got_hits, got_state = T.track_rows_np(frames, opt, state)
    assert got_rows.dtype == np.float32 and got_ids.dtype == np.int32 and got_hits.dtype == np.int32
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_hits, want_hits)
    assert O.same_state(want_state, got_state)
    cols = [c for c in range(36) if c != 25 or not opt['smooth']]
    assert np.array_equal(got_rows[..., cols].view(np.uint32), want_rows[..., cols].view(np.uint32))       # bit for bit, NaN included
    close = np.abs(got_rows[..., 25].astype(np.float64) - want_rows[..., 25]) <= 4 * np.spacing(np.abs(want_rows[..., 25]))
    assert (close | (got_rows[..., 25].view(np.uint32) == want_rows[..., 25].view(np.uint32))).all()
    return got_rows, got_ids, got_hits, got_state


@pytest.mark.parametrize('name,frames,opt', EXACT, ids=ids_of(EXACT))
def test_host_form_equals_the_oracle_on_the_exact_cases(name, frames, opt):
    to_thr, _ = O.margins(O.frame_values(frames, opt), opt)
    assert to_thr > 1e-9, to_thr                       # (no candidate sits on the threshold; equal candidates are wanted here)
    same_as_oracle(frames, opt)


@pytest.mark.parametrize('name,frames,opt', MARGIN, ids=ids_of(MARGIN))
def test_host_form_equals_the_oracle_where_the_margins_hold(name, frames, opt):
    """ what lets the GPU test ask for equality: no value within 1e-9 of the threshold, no two candidates of a frame within 1e-9 of
    each other -- an ulp of cos / sin cannot change a decision """
    to_thr, apart = O.margins(O.frame_values(frames, opt), opt)
    assert to_thr > 1e-9 and apart > 1e-9, (to_thr, apart)
    same_as_oracle(frames, opt)


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('metric', T.METRICS)
def test_seeded_scenes_equal_the_oracle(seed, metric):
    """ crowded lanes (3 m apart, thresholds that let neighbours compete), chunked in two with the state carried over """
    frames = O.drive(seed, frames=8, cars=8, D=12, noise=0.3, lane=3.0)
    opt = O.options(metric, threshold=4.0 if metric == 'dist' else 0.05, max_age=1, gains=(0.7, 0.2, 0.4), birth_score=0.4, smooth=True)
    to_thr, apart = O.margins(O.frame_values(frames, opt), opt)
    assert to_thr > 1e-12 and apart > 1e-12
    rows, ids, hits, state = same_as_oracle(frames, opt)
    _, _, _, ohalf = O.track(frames[:3], opt)
    _, _, _, half = T.track_rows_np(frames[:3], opt)
    rows2, ids2, hits2, state2 = same_as_oracle(frames[3:], opt, half, ohalf)
    assert np.array_equal(ids2, ids[3:]) and np.array_equal(hits2, hits[3:]) and state2.tobytes() == state.tobytes()
    assert rows2.tobytes() == rows[3:].tobytes()


def test_the_cases_say_what_the_issue_says():
    case = {c[0]: c for c in EXACT + MARGIN}
    run = lambda name: T.track_rows_np(*case[name][1:])  # noqa: E731
    for metric in T.METRICS:
        ids = run('crossing_' + metric)[1]
        assert set(ids[:, :2].ravel().tolist()) == {0, 1} and (ids[:, 2] == -1).all()
        assert run('gap_max_age_' + metric)[1][:, 0].tolist() == [0, 0, 0, -1, -1, 0, 0]            # the id survives max_age misses
        assert run('gap_max_age_plus_1_' + metric)[1][:, 0].tolist() == [0, 0, 0, -1, -1, -1, 1, 1]
        assert run('tie_rows_' + metric)[1].tolist() == [[0, -1], [0, 1]]                           # the smaller row wins
        _, ids, hits, state = run('tie_slots_' + metric)
        assert ids.tolist() == [[0, 1], [0, -1]] and hits[1].tolist() == [2, 0] and state['misses'][:2].tolist() == [0, 1]
        _, ids, hits, _ = run('odd_rows_' + metric)
        assert ids.tolist() == [[-1, 0, -1, 1], [-1, -1, 1, 0], [-1] * 4, [0, 1, -1, -1]] and hits[3].tolist() == [3, 3, 0, 0]
        assert run('birth_score_' + metric)[1][:, 1].tolist() == [-1] * 9                          # 0.8 < birth_score
        rows, ids, _, state = run('turned_' + metric)
        assert ids.tolist() == [[0, 1]] * 3
        ry = state['box'][3][:2]
        assert abs(ry[0] - 0.3) < 0.02 and abs(abs(ry[1]) - math.pi) < 0.03                         # neither moved toward the flipped reading
    for metric in ('dist', 'bev'):
        _, ids, hits, state = run('full_house_' + metric)
        assert ids[0].tolist() == list(range(128)) and ids[1].tolist() == list(range(127)) + [-1]
        assert int(state['dropped']) == 1 and int(state['next_id']) == 128 and int(state['misses'][127]) == 1
    crossing = case['crossing_dist'][1]
    assert O.margins(O.frame_values(crossing, O.options('dist')), O.options('dist'))[1] == 0.0      # equal candidates do occur there


def test_long_scene_has_no_switch():
    """ 6 cars further apart than twice the threshold, 30 frames, constant velocity, 5 cm noise, each missing at most max_age frames """
    frames, gts = O.drive(5, frames=30, cars=6, D=8, noise=0.05, max_age=2, lane=6.0, with_gt=True)
    assert any((g < 0).sum() > 2 for g in gts)                               # cars do go missing
    opt = {'metric': 'dist', 'threshold': 2.0, 'max_age': 2}
    _, ids, hits, state = T.track_rows_np(frames, opt)
    assert T.id_switches(gts, ids) == 0
    assert sorted(set(ids[ids >= 0].tolist())) == list(range(6)) and int(state['next_id']) == 6 and int(state['frames']) == 30
    assert ((ids >= 0) == (np.stack(gts) >= 0)).all()
    _, oids, _, ostate = O.track(frames, T.check_option(opt))
    assert np.array_equal(ids, oids) and O.same_state(ostate, state)


def test_empty_inputs_leave_the_state():
    frames = O.crossing()
    _, _, _, state = T.track_rows_np(frames[:2], ('dist', 2.3))
    for empty in (np.zeros((0, 3, 36), np.float32), np.zeros((2, 0, 36), np.float32)):
        rows, ids, hits, after = T.track_rows_np(empty, ('dist', 2.3), state)
        assert rows.shape == empty.shape and ids.shape == empty.shape[:2] and after.tobytes() == state.tobytes()
    assert T.empty_state().tobytes() == bytes(T.STATE_DTYPE.itemsize)
    assert T.read_state(state.tobytes()).tobytes() == state.tobytes()
    assert [t['id'] for t in T.tracks_of(state)] == [0, 1]


# ---------------------------------------------------------------------------------------------------- header and contract
def test_header_constants_and_contract():
    text = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    define = lambda name: int(re.search(r'#define {}\s+(\d+)'.format(name), text).group(1))  # noqa: E731
    assert [define('GPP_TRACK_' + m.upper()) for m in T.METRICS] == [0, 1, 2]
    assert define('GPP_TRACK_MAX_TRACKS') == T.MAX_TRACKS == hip.GPP_TRACK_MAX_TRACKS == O.T
    assert define('GPP_TRACK_FIELDS') == len(T.FIELDS) == hip.GPP_TRACK_FIELDS
    assert ctypes.sizeof(hip.TrackState) == T.STATE_DTYPE.itemsize == 12304
    for name, _ in hip.TrackState._fields_:
        assert getattr(hip.TrackState, name).offset == T.STATE_DTYPE.fields[name][1], name
    struct = text[text.index('typedef struct gpp_track_state'):text.index('} gpp_track_state;')]
    assert [m for m in re.findall(r'(\w+)\s*(?:\[[^;]*)?;', re.sub(r'/\*.*?\*/', '', struct))] == list(T.STATE_DTYPE.names)
    contract = ' '.join(text[text.index('Tracking of cuboids across frames'):text.index('#define GPP_TRACK_BEV')].split())
    for phrase in ('A state of all zero bytes is the empty tracker', 'ties to the smaller slot, then to the smaller row',
                   'overlap > threshold (strict)', 'q < threshold * threshold', 'misses > max_age', 'rows_out == rows_in is allowed',
                   'they may be the same buffer', 'GPP_ERR_UNSUPPORTED', 'reads all it needs of a frame before it writes'):
        assert phrase in contract, phrase
    makefile = open(os.path.join(ROOT, 'ground-plane-polling_amd', 'csrc', 'Makefile')).read()
    assert 'track.hip' in re.search(r'SRCS_EXACT = (.*)', makefile).group(1)


BAD_OPTIONS = [('iou', 0.3), ('bev', 1.0), ('3d', -0.1), ('bev', float('nan')), ('dist', 0.0), ('dist', float('inf')), ('dist', float('nan')),
               ('bev',), 5, {'metric': 'dist'}, {'metric': 'dist', 'threshold': 2.0, 'age': 1},
               {'metric': 'dist', 'threshold': 2.0, 'gains': (0.0, 0.1, 0.1)}, {'metric': 'dist', 'threshold': 2.0, 'gains': (0.5, 1.5, 0.1)},
               {'metric': 'dist', 'threshold': 2.0, 'gains': (0.5, 0.1, -0.1)}, {'metric': 'dist', 'threshold': 2.0, 'gains': (0.5, 0.1)},
               {'metric': 'dist', 'threshold': 2.0, 'gains': (0.5, float('nan'), 0.1)}, {'metric': 'dist', 'threshold': 2.0, 'max_age': -1},
               {'metric': 'dist', 'threshold': 2.0, 'max_age': 1.5}, {'metric': 'dist', 'threshold': 2.0, 'birth_score': float('nan')}]


@pytest.mark.parametrize('option', BAD_OPTIONS, ids=[str(k) for k in range(len(BAD_OPTIONS))])
def test_check_option_refuses(option):
    with pytest.raises(ValueError):
        T.check_option(option)


def test_check_option_accepts():
    assert T.check_option(None) is None
    assert T.check_option(('bev', 0)) == dict(T.DEFAULTS, metric='bev', threshold=0.0)
    full = {'metric': 'dist', 'threshold': 2.0, 'max_age': 0, 'gains': (1.0, 0.0, 1.0), 'birth_score': -1.0, 'smooth': True}
    assert T.check_option(full) == full and T.check_option(T.check_option(full)) == full


def bad_params():
    """ [(what, TrackParams, seq_start, D, code)] of include/gpp.h's error list """
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
    """ host code: every pointer is a host buffer nobody may touch -- a refusal returns before it is looked at """
    lib = hip.lib()
    seq = (ctypes.c_int32 * len(seq))(*seq)
    rc = lib.gpp_track_f64(None, 4, D, seq, len(seq) - 1, None, None, ctypes.byref(params), None, None, None, None, 0, None)
    assert rc == code


def test_c_abi_sizes():
    assert hip.track_state_bytes() == T.STATE_DTYPE.itemsize
    assert hip.track_workspace_bytes(0) == 256 and hip.track_workspace_bytes(3) == 256 + 3 * 2 * 128 * 128 * 8
    n = ctypes.c_size_t(0)
    assert hip.lib().gpp_track_workspace_bytes(-1, ctypes.byref(n)) == -1 and hip.lib().gpp_track_state_bytes(None) == -1
    good = hip.TrackParams(2, 2, 0, 0, 2.0, 0.5, 0.25, 0.25, 0.0)
    seq = (ctypes.c_int32 * 2)(0, 4)
    assert hip.lib().gpp_track_f64(None, 4, 4, None, 1, None, None, ctypes.byref(good), None, None, None, None, 0, None) == -1
    assert hip.lib().gpp_track_f64(None, 4, 4, seq, 1, None, None, None, None, None, None, None, 0, None) == -1
    assert hip.lib().gpp_track_f64(None, 4, 4, seq, 0, None, None, ctypes.byref(good), None, None, None, None, 0, None) == 0     # S == 0


# ---------------------------------------------------------------------------------------------------- text and switches
def test_tracking_lines_format():
    rows = np.stack([O.row(0.9, 1.0, 20.0), O.padding()[0], O.row(0.75, -2.5, 31.25, ry=-0.5), O.row(0.5, 0.0, 10.0)])
    text = T.tracking_lines(7, rows, [3, -1, 12, 4], [2, 0, 5, 1], min_hits=2)
    assert text == ('7 3 Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 1.00 1.65 20.00 0.00 0.90\n'
                    '7 12 Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 -2.50 1.65 31.25 -0.50 0.75\n')
    assert T.tracking_lines(7, rows, [3, -1, 12, 4], [2, 0, 5, 1]).count('\n') == 3
    assert T.tracking_lines(0, rows, [-1] * 4, [0] * 4) == ''
    for line in text.splitlines():
        assert len(line.split()) == 18


def test_id_switches():
    assert T.id_switches([], []) == 0
    assert T.id_switches([[0, 1], [1, 0], [0, 1]], [[5, 6], [6, 5], [5, 6]]) == 0              # the rows move, the ids stay
    assert T.id_switches([[0, 1], [0, 1]], [[5, 6], [6, 5]]) == 2
    assert T.id_switches([[0], [0], [0]], [[5], [-1], [5]]) == 0                               # a miss is no switch
    assert T.id_switches([[0], [0], [0]], [[5], [-1], [7]]) == 1
    assert T.id_switches([[-1, 0], [0, -1]], [[9, 5], [5, 8]]) == 0                            # rows of no object do not count


# ---------------------------------------------------------------------------------------------------- model and command lines
def test_model_option_errors_come_before_the_device():
    from keras_retinanet_3D import models
    from keras_retinanet_3D.models import weights as W
    w = W.synthetic_weights('resnet50', 1)
    with pytest.raises(ValueError, match='needs pose=True'):
        models.load_model(w, backbone_name='resnet50', track=('dist', 2.0))
    with pytest.raises(ValueError, match='metric'):
        models.load_model(w, backbone_name='resnet50', pose=True, track=('iou', 0.3))
    with pytest.raises(ValueError, match='finite and positive'):
        models.load_model(w, backbone_name='resnet50', pose=True, track={'metric': 'dist', 'threshold': 0.0})


def test_pipeline_and_sharded_model_refuse_a_track_model():
    import types
    from keras_retinanet_3D.utils.distributed import ShardedModel
    from keras_retinanet_3D.utils.pipeline import FramePipeline
    model = types.SimpleNamespace(audit=False, track=T.check_option(('dist', 2.0)))
    with pytest.raises(ValueError, match='track'):
        FramePipeline(model)
    with pytest.raises(ValueError, match='track'):
        ShardedModel(model)


def test_command_line_arguments(tmp_path):
    from keras_retinanet_3D.bin import run_network, track_results
    base = ['m.h5', 'img', 'calib', 'planes.mat', 'out']
    args = run_network.parse_args(base + ['--device-pose', '--track', 'bev', '--track-threshold', '0.1', '--track-max-age', '3', '--track-smooth'])
    assert run_network.track_option(args) == {'metric': 'bev', 'threshold': 0.1, 'max_age': 3, 'smooth': True} and args.track_min_hits == 1
    assert run_network.track_option(run_network.parse_args(base)) is None
    for bad in (['--track', 'dist', '--track-threshold', '2'], ['--device-pose', '--track', 'dist'], ['--device-pose', '--track-threshold', '2'],
                ['--device-pose', '--track', 'bev', '--track-threshold', '1.0'], ['--device-pose', '--track', 'dist', '--track-threshold', '0'],
                ['--device-pose', '--track', 'dist', '--track-threshold', '2', '--track-max-age', '-1'],
                ['--device-pose', '--save-images', '--track', 'dist', '--track-threshold', '2']):
        with pytest.raises(SystemExit):
            run_network.parse_args(base + bad)
    with pytest.raises(SystemExit):
        track_results.parse_args(['dir', 'tracks.txt', '--metric', 'bev', '--threshold', '1.5'])
    # in_order: only neighbours share a call
    items = [{'raw_image': np.zeros(s, np.uint8)} for s in ((4, 6, 3), (4, 6, 3), (5, 6, 3), (4, 6, 3))]
    model = type('M', (), {'supports_ragged': False})()
    assert [len(g) for g, _ in run_network.group_items(model, items)] == [3, 1]
    groups = run_network.group_items(model, items, in_order=True)
    assert [len(g) for g, _ in groups] == [2, 1, 1] and [it for g, _ in groups for it in g] == items
    # the host path of track_results.py: two frames, one car that moves, one that appears
    line = 'Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 {:.2f} 1.65 {:.2f} 0.00 {:.2f}\n'
    (tmp_path / 'r').mkdir()
    (tmp_path / 'r' / '000000.txt').write_text(line.format(1.0, 20.0, 0.9))
    (tmp_path / 'r' / '000001.txt').write_text(line.format(-8.0, 30.0, 0.8) + line.format(1.5, 20.5, 0.7))
    track_results.main([str(tmp_path / 'r'), str(tmp_path / 't.txt'), '--metric', 'dist', '--threshold', '2', '--host'])
    assert (tmp_path / 't.txt').read_text() == '0 0 ' + line.format(1.0, 20.0, 0.9) + '1 1 ' + line.format(-8.0, 30.0, 0.8) + \
        '1 0 ' + line.format(1.5, 20.5, 0.7)
