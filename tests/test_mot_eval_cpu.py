""" CPU tests of the tracking score: the NumPy form (utils/mot_eval.py) against the loop-written oracle
(tests/mot_oracle.py) on the issue's cases and on seeded scenes; the assignment's total cost against scipy's linear_sum_assignment; the
header's constants; the C ABI's argument checks (host code: they come before any launch); the files and the command lines. """
import ctypes
import json
import os
import re

import numpy as np
import pytest

import mot_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import mot_eval as M
from keras_retinanet_3D.utils import track as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = O.named_cases()
SCENES = [('scene_{}'.format(s), O.scene(s, frames=6, cars=5 + s, quantum=q)) for s, q in ((1, 8.0), (2, 16.0), (3, 32.0), (4, 4.0))] + \
         [('dense_{}_{}'.format(g, t), O.dense(g + t, g, t)) for g, t in ((1, 1), (9, 4), (4, 9), (17, 17), (24, 31))] + \
         [('far', O.dense(5, 6, 5, far=True))]


def same_as_oracle(labels, tracks, **options):
    """ every integer of the NumPy form against the oracle's; -> the NumPy form's result """
    got = M.evaluate_sequences(labels, tracks, **options)
    want = O.evaluate(labels, tracks, **options)
    for s, (seq, table) in enumerate(zip(want['sequences'], want['tables'])):
        assert {k: got['sequences'][s][k] for k in O.COUNT_NAMES} == seq
        traj = got['trajectories'][s]
        seen = traj['table'][:, 0] > 0
        assert {int(i): line.tolist() for i, line in zip(traj['track_ids'][seen], traj['table'][seen])} == table
        f0 = int(got['seq_start'][s])
        for f, (match, lout, rout, counts) in enumerate(want['frames'][s]):
            assert got['frames']['match'][f0 + f, :len(match)].tolist() == match
            assert got['frames']['label_outcome'][f0 + f, :len(lout)].tolist() == lout
            assert got['frames']['row_outcome'][f0 + f, :len(rout)].tolist() == rout
            assert got['frames']['counts'][f0 + f].tolist() == counts
    total = {k: sum(seq[k] for seq in want['sequences']) for k in O.COUNT_NAMES}
    assert {k: got['all'][k] for k in O.COUNT_NAMES} == total
    return got, want


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_cases_equal_the_oracle_and_say_what_the_issue_says(name):
    labels, tracks, expect, options = CASES[name]
    got, _ = same_as_oracle(labels, tracks, **options)
    for key, value in expect.items():
        assert got['sequences'][0][key] == value, (key, got['sequences'][0][key], value)
        assert got['all'][key] == value, key


def test_optimal_beats_greedy():
    labels, tracks, _, _ = CASES['optimal_beats_greedy']
    got, want = same_as_oracle(labels, tracks)
    cost = want['costs'][0][0]
    assert [[c < O.BIG for c in line] for line in cost] == [[True, True], [False, True]] and cost[0][1] < cost[0][0]
    assert O.greedy_pairs(cost) == 1 and got['all']['tp'] == 2                  # best-overlap-first takes (label 0, row 1) and strands label 1
    assert got['frames']['match'][0].tolist() == [0, 1]


def test_ties_take_the_first_index():
    labels, tracks, _, _ = CASES['ties']
    got, want = same_as_oracle(labels, tracks)
    cost = np.array(want['costs'][0][0])
    assert (cost == cost[0, 0]).all() and got['frames']['match'][0].tolist() == [0, 1] == want['frames'][0][0][0]


def test_threshold_is_not_strict():
    labels, tracks, _, _ = CASES['threshold']
    _, want = same_as_oracle(labels, tracks)
    assert want['costs'][0][0] == [[1 << 19]] and want['costs'][0][1] == [[O.BIG]]
    again, _ = same_as_oracle(labels, tracks, min_overlap=0.5 - 2.0 ** -20)      # one quantum lower: both frames match
    assert again['all']['tp'] == 2 and again['all']['sum_k'] == (1 << 20) - 1


@pytest.mark.parametrize('name,scene', SCENES, ids=[s[0] for s in SCENES])
def test_seeded_scenes_equal_the_oracle(name, scene):
    labels, tracks = scene
    got, want = same_as_oracle([labels], [tracks])
    if name.startswith('scene'):
        assert got['all']['tp'] > 0 and got['all']['fn'] > 0
    if name == 'far':
        assert got['all']['tp'] == 0 and got['all']['fn'] == 6 and got['all']['fp'] == 5


def test_seeded_scenes_cover_the_rules():
    """ the scenes together reach every outcome code, switches and fragmentations """
    louts, routs, ids, frag = set(), set(), 0, 0
    for name, (labels, tracks) in SCENES[:4]:
        got = M.evaluate_sequences([labels], [tracks])
        louts |= set(got['frames']['label_outcome'].ravel().tolist())
        routs |= set(got['frames']['row_outcome'].ravel().tolist())
        ids, frag = ids + got['all']['ids'], frag + got['all']['frag']
    assert louts == {0, 1, 2, 3, 4} and routs == {0, 1, 2, 3, 4, 5} and ids > 0 and frag > 0


@pytest.mark.parametrize('metric', ['bev', '3d'])
def test_other_metrics_equal_the_oracle(metric):
    labels, tracks = O.scene(7, frames=4, cars=6)
    got, _ = same_as_oracle([labels], [tracks], metric=metric, min_overlap=0.25)
    assert got['all']['tp'] > 0


def test_several_sequences_sum():
    scenes = [O.scene(11, frames=5, cars=4), (([], []), ([], [])), O.scene(12, frames=3, cars=7)]
    got, _ = same_as_oracle([s[0] for s in scenes], [s[1] for s in scenes])
    assert got['seq_start'].tolist() == [0, 5, 5, 8] and got['sequences'][1]['frames'] == 0 and got['sequences'][1]['mota'] is None


# ---------------------------------------------------------------------------------------------------- optimality
def seeded_matrices():
    rng = np.random.default_rng(0)
    out = []
    for k in range(60):                                                        # rectangular, with ties, with inadmissible cells
        G, T = rng.integers(1, 14, 2)
        n = max(G, T)
        cost = np.full((n, n), M.BIG, np.int64)
        k_values = rng.integers(1 << 19, (1 << 20) + 1, (G, T)) if k % 2 else (rng.integers(4, 9, (G, T)) << 17)
        cost[:G, :T] = np.where(rng.random((G, T)) < 0.6, M.SCALE - k_values, M.BIG)
        out.append(cost)
    for name, (labels, tracks) in SCENES:
        out += [np.array(c, np.int64).reshape(len(c), len(c)) for c in O.evaluate([labels], [tracks])['costs'][0]]
    big = np.full((128, 128), M.BIG, np.int64)
    mask = rng.random((128, 128)) < 0.3
    big[mask] = M.SCALE - (rng.integers(4, 9, mask.sum()) << 17)
    return out + [big]


def test_total_cost_equals_scipy():
    optimize = pytest.importorskip('scipy.optimize')
    matrices = seeded_matrices()
    assert len(matrices) > 80
    for cost in matrices:
        col, total = M.assign_np(cost)
        assert sorted(col.tolist()) == list(range(cost.shape[0]))
        r, c = optimize.linear_sum_assignment(cost)
        assert total == int(cost[r, c].sum())
        if cost.shape[0] <= 14:
            assert col.tolist() == O.assign(cost.tolist())                     # the same algorithm: the same assignment, not only the same cost


# ---------------------------------------------------------------------------------------------------- header and ABI
def test_header_constants_and_contract():
    text = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    define = lambda name: int(eval(re.search(r'#define {}\s+(\(?[\d <]+\)?)'.format(name), text).group(1)))  # noqa: E731
    assert define('GPP_MOT_SCALE_BITS') == M.SCALE_BITS == hip.GPP_MOT_SCALE_BITS and M.SCALE == O.SCALE == 1 << 20
    assert define('GPP_MOT_BIG') == M.BIG == hip.GPP_MOT_BIG == O.BIG and 128 * M.SCALE < M.BIG
    assert define('GPP_MOT_MAX_TRAJECTORIES') == M.MAX_TRAJECTORIES == hip.GPP_MOT_MAX_TRAJECTORIES
    assert define('GPP_MOT_FRAME_COUNTS') == len(M.FRAME_COUNTS) == hip.GPP_MOT_FRAME_COUNTS
    assert define('GPP_MOT_SEQ_COUNTS') == hip.GPP_MOT_SEQ_COUNTS >= len(M.SEQ_COUNTS) and define('GPP_MOT_TRAJ_COLS') == hip.GPP_MOT_TRAJ_COLS == 4
    assert M.MAX_ROWS == define('GPP_KITTI_MAX_DETECTIONS') and M.MAX_LABELS == define('GPP_KITTI_MAX_LABELS')
    struct = text[text.index('typedef struct gpp_mot_params'):text.index('} gpp_mot_params;')]
    assert re.findall(r'(\w+);', re.sub(r'/\*.*?\*/', '', struct)) == [n for n, _ in hip.MotParams._fields_]
    assert ctypes.sizeof(hip.MotParams) == 40
    contract = ' '.join(text[text.index('CLEAR-MOT scoring of tracks on the device'):text.index('#define GPP_MOT_SCALE_BITS')].replace('\n *', '\n').split())
    for phrase in ('UNPINNED', 'o >= min_overlap (not strict', 'the FIRST column that has it', 'A pair whose cell is GPP_MOT_BIG is no pair',
                   'on the HOST', 'GPP_ERR_UNSUPPORTED', 'D == 0 is legal', 'A == 0 is legal'):
        assert phrase in contract, phrase
    makefile = open(os.path.join(ROOT, 'ground-plane-polling_amd', 'csrc', 'Makefile')).read()
    assert 'mot_eval.hip' in re.search(r'SRCS_EXACT = (.*)', makefile).group(1) and '$(OBJ)/mot_eval.o: mot_eval.hip' in makefile
    assert M.DEFAULTS == O.LIMITS and (M.COUNTING, M.IGNORED) == (0, 1)


def bad_assign_calls():
    good = dict(metric=0, reserved=0, min_overlap=0.5, max_occlusion=2.0, max_truncation=0.0, min_height=25.0)
    nan = float('nan')
    out = [(what, hip.MotParams(**dict(good, **change)), 4, 4, 4, -1) for what, change in [
        ('metric_3', dict(metric=3)), ('metric_negative', dict(metric=-1)), ('reserved', dict(reserved=1)), ('overlap_above', dict(min_overlap=1.5)),
        ('overlap_negative', dict(min_overlap=-0.1)), ('overlap_nan', dict(min_overlap=nan)), ('occlusion_nan', dict(max_occlusion=nan)),
        ('truncation_nan', dict(max_truncation=nan)), ('height_nan', dict(min_height=nan))]]
    g = hip.MotParams(**good)
    return out + [('n_negative', g, -1, 4, 4, -1), ('d_negative', g, 4, -1, 4, -1), ('a_negative', g, 4, 4, -1, -1), ('d_129', g, 4, 129, 4, -4),
                  ('a_129', g, 4, 4, 129, -4), ('null_pointers', g, 4, 4, 4, -1), ('nothing_to_do', g, 0, 4, 4, 0)]


@pytest.mark.parametrize('what,params,N,D,A,code', bad_assign_calls(), ids=[b[0] for b in bad_assign_calls()])
def test_assign_refuses_before_any_launch(what, params, N, D, A, code):
    """ host code: every pointer is null -- a refusal returns before it is looked at """
    assert hip.lib().gpp_mot_assign(None, None, None, None, None, N, D, A, ctypes.byref(params), None, None, None, None, None) == code


def test_assign_refuses_null_params():
    assert hip.lib().gpp_mot_assign(None, None, None, None, None, 4, 4, 4, None, None, None, None, None, None) == -1


CLEAR_CALLS = [('seq_descending', 4, 4, 4, [3, 2], 8, -1), ('seq_beyond', 4, 4, 4, [0, 5], 8, -1), ('seq_negative', 4, 4, 4, [-1, 4], 8, -1),
               ('n_negative', -1, 4, 4, [0, 0], 8, -1), ('traj_negative', 4, 4, 4, [0, 4], -1, -1), ('d_129', 4, 129, 4, [0, 4], 8, -4),
               ('a_129', 4, 4, 129, [0, 4], 8, -4), ('traj_beyond_the_cap', 4, 4, 4, [0, 4], 1025, -4), ('null_pointers', 4, 4, 4, [0, 4], 8, -1),
               ('no_sequence', 4, 4, 4, [0], 8, 0)]


@pytest.mark.parametrize('what,N,D,A,seq,max_traj,code', CLEAR_CALLS, ids=[c[0] for c in CLEAR_CALLS])
def test_clear_refuses_before_any_launch(what, N, D, A, seq, max_traj, code):
    seq_start = (ctypes.c_int32 * len(seq))(*seq)
    rc = hip.lib().gpp_mot_clear(None, None, None, None, None, N, D, A, seq_start, len(seq) - 1, max_traj, None, None, None, 0, None)
    assert rc == code


def test_clear_sizes():
    n = ctypes.c_size_t(0)
    assert hip.mot_clear_workspace_bytes(0) == 256 and hip.mot_clear_workspace_bytes(63) == 256 and hip.mot_clear_workspace_bytes(64) == 512
    assert hip.lib().gpp_mot_clear_workspace_bytes(-1, ctypes.byref(n)) == -1 and hip.lib().gpp_mot_clear_workspace_bytes(1, None) == -1
    assert hip.lib().gpp_mot_clear(None, None, None, None, None, 4, 4, 4, None, 1, 8, None, None, None, 0, None) == -1      # no seq_start


# ---------------------------------------------------------------------------------------------------- host-side errors, files, command lines
def test_duplicates_are_value_errors():
    labs, tids = O.two_cars(2)
    rows = [O.rows_of(g) for g in labs]
    ids = [np.array([7, 9])] * 2
    with pytest.raises(ValueError, match='track_id labels two objects'):
        M.evaluate_sequences([(labs, [np.array([3, 3]), np.array([3, 5])])], [(rows, ids)])
    with pytest.raises(ValueError, match='tracker id appears twice'):
        M.evaluate_sequences([(labs, tids)], [(rows, [np.array([7, 9]), np.array([9, 9])])])
    dc = [np.stack([O.label(2, (0.0, 0.0, 50.0, 50.0))] * 2)] * 2                 # DontCare regions all carry -1: no duplicate
    assert M.evaluate_sequences([(dc, [np.array([-1, -1])] * 2)], [(rows, ids)])['all']['fp'] == 4
    padded = [np.concatenate([r, np.full((1, 36), -1.0, np.float32)]) for r in rows]
    assert M.evaluate_sequences([(labs, tids)], [(padded, [np.array([7, 9, 9])] * 2)])['all']['tp'] == 4       # a padding row's id is not read
    for bad in (dict(metric='iou'), dict(min_overlap=1.5), dict(min_overlap=float('nan')), dict(min_height=float('nan'))):
        with pytest.raises(ValueError):
            M.evaluate_sequences([(labs, tids)], [(rows, ids)], **bad)
    with pytest.raises(ValueError, match='at most 128'):
        M.evaluate_sequences([O.dense(0, 129, 1)[0]], [O.dense(0, 129, 1)[1]])


def write_scene(tmp_path, name, labels, tracks):
    (tmp_path / 'label_02').mkdir(exist_ok=True)
    (tmp_path / 'tracks').mkdir(exist_ok=True)
    kinds = {0: 'Car', 1: 'Van', 2: 'DontCare', 3: 'Pedestrian'}
    with open(str(tmp_path / 'label_02' / name), 'w') as f:
        for k, (g, t) in enumerate(zip(*labels)):
            for line, tid in zip(g, t):
                f.write('{} {} {} {:g} {:g} '.format(k, int(tid), kinds[int(line[0])], line[1], line[2]) + ' '.join(repr(float(v)) for v in line[3:15]) + '\n')
    with open(str(tmp_path / 'tracks' / name), 'w') as f:
        for k, (r, i) in enumerate(zip(*tracks)):
            f.write(T.tracking_lines(k, r, i, np.ones(len(i), np.int32)))


def test_files_round_trip_and_command_line(tmp_path, capsys):
    from keras_retinanet_3D.bin import evaluate_tracking
    labels, tracks = O.scene(21, frames=5, cars=5)
    write_scene(tmp_path, '0000.txt', labels, tracks)
    write_scene(tmp_path, '0001.txt', *O.scene(22, frames=3, cars=4))
    rows, ids = M.read_track_file(str(tmp_path / 'tracks' / '0000.txt'))          # tracking_lines -> read_track_file
    assert len(rows) == 5 and all(np.array_equal(i, j) for i, j in zip(ids, tracks[1]))
    for r, want in zip(rows, tracks[0]):
        assert np.array_equal(r[:, 26:30], want[:, 26:30]) and (r[:, 14] == 0).all()    # (boxes on the grid survive two decimals)
    labs, tids = M.read_tracking_labels(str(tmp_path / 'label_02' / '0000.txt'))
    assert all(np.array_equal(a, b) for a, b in zip(labs, labels[0])) and all(np.array_equal(a, b) for a, b in zip(tids, labels[1]))
    direct = M.evaluate_sequences([labels], [tracks])
    single = M.evaluate_tracking(str(tmp_path / 'label_02' / '0000.txt'), str(tmp_path / 'tracks' / '0000.txt'))
    assert single['all'] == direct['all'] and single['names'] == ['0000']
    result = evaluate_tracking.main([str(tmp_path / 'label_02'), str(tmp_path / 'tracks'), '--json', str(tmp_path / 'out.json')])
    assert result['names'] == ['0000', '0001'] and result['sequences'][0] == direct['all']
    text = capsys.readouterr().out
    assert text.startswith('CLEAR-MOT, Car, image overlap >= 0.5') and len(text.strip().splitlines()) == 5 and ' all ' in text
    saved = json.load(open(str(tmp_path / 'out.json')))
    assert saved['all'] == result['all'] and set(saved['sequences']) == {'0000', '0001'}
    os.remove(str(tmp_path / 'tracks' / '0001.txt'))                               # a missing track file: a sequence without tracks
    missing = M.evaluate_tracking(str(tmp_path / 'label_02'), str(tmp_path / 'tracks'))
    assert missing['sequences'][1]['tp'] == 0 and missing['sequences'][1]['fn'] == missing['sequences'][1]['n_gt'] > 0
    for bad in (['a', 'b', '--metric', 'iou'], ['a', 'b', '--min-overlap', '1.5'], [str(tmp_path / 'label_02'), str(tmp_path / 'out.json')], ['a']):
        with pytest.raises(SystemExit):
            evaluate_tracking.parse_args(bad)
    with pytest.raises(ValueError, match='17 fields'):
        (tmp_path / 'bad.txt').write_text('0 1 Car 0 0\n')
        M.read_tracking_labels(str(tmp_path / 'bad.txt'))


def test_tracking_command_lines_take_labels(tmp_path, capsys):
    from keras_retinanet_3D.bin import run_network, track_results
    base = ['m.h5', 'img', 'calib', 'planes.mat', 'out']
    args = run_network.parse_args(base + ['--device-pose', '--track', 'dist', '--track-threshold', '2', '--tracking-labels', 'l.txt'])
    assert args.tracking_labels == 'l.txt' and run_network.parse_args(base).tracking_labels is None
    with pytest.raises(SystemExit):
        run_network.parse_args(base + ['--device-pose', '--tracking-labels', 'l.txt'])
    with pytest.raises(SystemExit):
        track_results.parse_args(['dir', 't.txt', '--metric', 'dist', '--threshold', '2', '--score-min-overlap', '2'])
    # the host path of track_results.py --labels: one car in two frames, found in both
    line = 'Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 {:.2f} 1.65 {:.2f} 0.00 {:.2f}\n'
    (tmp_path / 'r').mkdir()
    (tmp_path / 'r' / '000000.txt').write_text(line.format(1.0, 20.0, 0.9))
    (tmp_path / 'r' / '000001.txt').write_text(line.format(1.5, 20.5, 0.7))
    (tmp_path / 'l.txt').write_text(''.join('{} 4 Car 0 0 0.25 100 100 200 180 1.5 2 3 1 1.65 20 0\n'.format(k) for k in range(2)))
    result = track_results.main([str(tmp_path / 'r'), str(tmp_path / 't.txt'), '--metric', 'dist', '--threshold', '2', '--host',
                                 '--labels', str(tmp_path / 'l.txt')])
    assert result['all']['tp'] == 2 and result['all']['mota'] == 1.0 and result['all']['motp'] == 1.0 and result['all']['mt'] == 1
    assert 'CLEAR-MOT, Car, image overlap >= 0.5' in capsys.readouterr().out
