""" CPU tests of HOTA: the NumPy form (utils/hota_eval.py) against the loop-written oracle (tests/hota_oracle.py)
at every stage; hand-derived cases; the assignment's total against scipy's; the integer form against a float64 restatement of the
metric's definition; the opt-in leaves today's result alone; the ValueErrors; the command lines; the C ABI's argument checks (host code:
they come before any launch). """
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import hota_oracle as HO
import mot_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import hota_eval as H
from keras_retinanet_3D.utils import mot_eval as M
from keras_retinanet_3D.utils import pair_tables as PT
from test_mot_eval_cpu import write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = O.named_cases()
S = 1 << 20
SCENES = [('scene_{}_{}'.format(seed, k), O.scene(seed, **kw)) for k, (seed, kw) in enumerate(HO.SCENES)] + \
         [('dense_{}_{}'.format(g, t), O.dense(g + t, g, t)) for g, t in ((1, 1), (9, 4), (4, 9), (24, 31))] + \
         [('far', O.dense(5, 6, 5, far=True))]
_RESULTS = {}


def scored(name):
    """ (labels, tracks, the NumPy form's result, the oracle's), computed once per scene """
    if name not in _RESULTS:
        labels, tracks = dict(SCENES)[name]
        _RESULTS[name] = ([labels], [tracks], M.evaluate_sequences([labels], [tracks], hota=True), HO.evaluate([labels], [tracks]))
    return _RESULTS[name]


def same_as_oracle(got, want, labels, tracks):
    """ every stage of the NumPy form against the oracle's dicts """
    for s, w in enumerate(want):
        pairs = got['hota_pairs'][s]
        track_ids = got['trajectories'][s]['track_ids']
        rows, ids = tracks[s]
        live = [int(i) for r, ii in zip(rows, ids) for i, x in zip(np.asarray(ii).reshape(-1), np.asarray(r).reshape(-1, 36)) if x[14] >= 0 and i >= 0]
        tracker_ids = sorted(set(live))
        assert pairs['P'].dtype == np.int64 and pairs['A'].dtype == np.int32 and pairs['hist'].dtype == np.int32
        assert pairs['gc'].dtype == np.int32 and pairs['tc'].dtype == np.int32
        assert pairs['P'].shape == (len(track_ids), len(tracker_ids)) and pairs['hist'].shape == pairs['P'].shape + (20,)
        P = {(int(g), t): int(pairs['P'][i, j]) for i, g in enumerate(track_ids) for j, t in enumerate(tracker_ids)}
        assert {k: v for k, v in P.items() if v} == {k: v for k, v in w['P'].items() if v}
        A = {(int(g), t): int(pairs['A'][i, j]) for i, g in enumerate(track_ids) for j, t in enumerate(tracker_ids)}
        assert {k: v for k, v in A.items() if v} == {k: v for k, v in w['A'].items() if v}
        assert {int(g): int(n) for g, n in zip(track_ids, pairs['gc']) if n} == w['gc']
        assert {t: int(n) for t, n in zip(tracker_ids, pairs['tc']) if n} == w['tc']
        hist = {(int(g), t): pairs['hist'][i, j].tolist() for i, g in enumerate(track_ids) for j, t in enumerate(tracker_ids) if pairs['hist'][i, j].any()}
        assert hist == w['hist']
        f0 = int(got['seq_start'][s])
        for f, fr in enumerate(w['frames']):
            assert got['hota_frames']['match'][f0 + f, :len(fr['match'])].tolist() == fr['match']
            assert (got['hota_frames']['match'][f0 + f, len(fr['match']):] == -1).all()
            assert got['hota_frames']['counts'][f0 + f].tolist() == fr['counts']
        assert got['sequences'][s]['hota']['integers'] == w['ints']
    total = {name: [sum(w['ints'][name][j] for w in want) for j in range(19)] for name in HO.NAMES}
    assert got['all']['hota']['integers'] == total
    assert got['hota_frames']['match'].dtype == np.int32 and got['hota_frames']['counts'].dtype == np.int64


# ---------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize('name', [n for n, _ in SCENES])
def test_every_stage_equals_the_oracle(name):
    labels, tracks, got, want = scored(name)
    same_as_oracle(got, want, labels, tracks)
    if name.startswith('scene'):
        assert got['all']['hota']['integers']['tp'][0] > 0 and 0.0 < got['all']['hota']['hota'] < 1.0


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_cases_equal_the_oracle(name):
    labels, tracks, _, options = CASES[name]
    got = H.evaluate_hota_sequences(labels, tracks, **options)
    same_as_oracle(got, HO.evaluate(labels, tracks, **options), labels, tracks)


@pytest.mark.parametrize('metric', ['bev', '3d'])
def test_other_metrics_equal_the_oracle(metric):
    labels, tracks = O.scene(7, frames=4, cars=6)
    got = H.evaluate_hota_sequences([labels], [tracks], metric=metric, min_overlap=0.25)
    same_as_oracle(got, HO.evaluate([labels], [tracks], metric=metric, min_overlap=0.25), [labels], [tracks])
    assert got['all']['hota']['integers']['tp'][0] > 0


def test_several_sequences_sum():
    scenes = [O.scene(41, frames=17, cars=9, quantum=16.0), (([], []), ([], [])), O.scene(42, frames=5, cars=20), O.dense(3, 30, 40)]
    labels, tracks = [s[0] for s in scenes], [s[1] for s in scenes]
    got = H.evaluate_hota_sequences(labels, tracks)
    same_as_oracle(got, HO.evaluate(labels, tracks), labels, tracks)
    assert all(v is None for k, v in got['sequences'][1]['hota'].items() if k in H.RATIOS) and got['all']['hota']['hota'] > 0


# ---------------------------------------------------------------------------------------------------- hand-derived cases
def every(h, **want):
    for key, value in want.items():
        assert h['thresholds'][key] == [value] * 19 and h[key] == pytest.approx(value, abs=1e-15), key


def test_perfect():
    labels, tracks, _, _ = CASES['perfect']
    h = H.evaluate_hota_sequences(labels, tracks)['all']['hota']
    assert h['integers']['tp'] == [10] * 19 and h['integers']['fn'] == h['integers']['fp'] == [0] * 19
    every(h, hota=1.0, deta=1.0, assa=1.0, loca=1.0, detre=1.0, detpr=1.0, assre=1.0, asspr=1.0)


def test_split():
    """ one car under id 7 and then id 9, three frames each: per id mc = 3, gc = 6, tc = 3 -- ASS = 2 floor(9 S / 6) = 3 S over TP = 6 """
    labels, tracks = HO.split_case()
    got = M.evaluate_sequences(labels, tracks, hota=True)
    h = got['all']['hota']
    assert h['integers']['tp'] == [6] * 19 and h['integers']['ass'] == [3 * S] * 19
    every(h, deta=1.0, assa=0.5, assre=0.5, asspr=1.0, hota=math.sqrt(0.5), loca=1.0)
    assert got['all']['mota'] == 1.0 - 1.0 / 6.0 and got['all']['ids'] == 1


def test_swap():
    """ two cars whose ids change hands after frame 3 of 5: gc = tc = 5 everywhere; the two pairs seen three times give
    floor(9 S / (5 + 5 - 3)) each, the two seen twice floor(4 S / (5 + 5 - 2)) """
    labels, tracks, _, _ = CASES['swap']
    h = H.evaluate_hota_sequences(labels, tracks)['all']['hota']
    assert h['integers']['tp'] == [10] * 19
    assert h['integers']['ass'] == [2 * ((9 * S) // 7) + 2 * ((4 * S) // 8)] * 19


def test_alignment_breaks_a_tie():
    labels, tracks = HO.tie_case()
    got = M.evaluate_sequences(labels, tracks, hota=True)
    assert got['frames']['match'][3].tolist() == [0] and got['all']['ids'] == 1         # section 4.29: the first of two equal columns
    assert got['hota_frames']['match'][3].tolist() == [1]                               # section 4.30: the row the trajectory is aligned with
    h = got['all']['hota']
    assert h['integers']['tp'] == [4] * 19 and h['integers']['fp'] == [1] * 19 and h['integers']['fn'] == [0] * 19
    every(h, deta=0.8, assa=1.0)


def test_threshold():
    """ overlaps of exactly 0.5 and of one quantum below: both count up to j = 9, the first alone at j = 10, neither above """
    labels, tracks, _, _ = CASES['threshold']
    got = M.evaluate_sequences(labels, tracks, hota=True)
    assert got['all']['hota']['integers']['tp'] == [2] * 9 + [1] + [0] * 9
    assert (got['all']['tp'], got['all']['fp'], got['all']['fn']) == (1, 1, 1)
    assert got['all']['hota']['integers']['sq'][9] == S // 2 and got['all']['hota']['thresholds']['loca'][10:] == [1.0] * 9


def test_quantum_rule_at_the_double_nearest_06():
    """ jm = (20 q + 19) >> 20: the double nearest 0.6 (48 / 80) counts at j = 12, as the float rule s >= 0.6 - eps says """
    q = int(np.floor(48.0 / 80.0 * S))
    assert min(19, (20 * q + 19) >> 20) == 12 and 20 * q < 12 * S
    assert min(19, (20 * (S // 2) + 19) >> 20) == 10 and min(19, (20 * S + 19) >> 20) == 19 and (20 * ((S // 20) - 1) + 19) >> 20 == 0


def test_ignored_and_empty():
    labels, tracks, _, _ = CASES['ignored']
    h = H.evaluate_hota_sequences(labels, tracks)['all']['hota']
    assert all(h[name] is None and h['thresholds'][name] == [None] * 19 for name in H.RATIOS) and h['integers']['tp'] == [0] * 19
    labels, tracks, _, _ = CASES['empty']                      # sequence 0: a lone row and a lone label; sequence 1: no frames
    got = H.evaluate_hota_sequences(labels, tracks)
    assert all(got['sequences'][1]['hota'][name] is None for name in H.RATIOS)
    h = got['sequences'][0]['hota']
    assert h['integers']['fn'] == [1] * 19 and h['integers']['fp'] == [1] * 19 and h['deta'] == 0.0 and h['hota'] == 0.0 and h['loca'] == 1.0
    none = H.evaluate_hota_sequences([], [])
    assert all(none['all']['hota'][name] is None for name in H.RATIOS) and none['hota_pairs'] == []


# ---------------------------------------------------------------------------------------------------- optimality and the definition
@pytest.mark.parametrize('name', [n for n, _ in SCENES])
def test_total_cost_equals_scipy(name):
    from scipy.optimize import linear_sum_assignment
    _, _, _, want = scored(name)
    frames = 0
    for fr in want[0]['frames']:
        cost = np.array(fr['cost'], np.int64).reshape(len(fr['cost']), len(fr['cost']))
        if not cost.size:
            continue
        col, total = M.assign_np(cost)
        ri, ci = linear_sum_assignment(cost)
        assert total == int(cost[ri, ci].sum()) and col.tolist() == O.assign(cost.tolist())
        frames += 1
    assert frames > 0


@pytest.mark.parametrize('k', range(len(HO.SCENES)))
def test_integer_form_pins_the_definition(k):
    """ the integers against the float64 restatement: first the same pairs and TP_j, then DetA DetRe DetPr within 1e-12, AssA AssRe AssPr
    LocA within 2^-20 (every term is a mean of quantities floored once at 2^-20), HOTA_j^2 within 2^-19 """
    name = [n for n, _ in SCENES][k]
    labels, tracks, got, _ = scored(name)
    ref = HO.float_hota(labels, tracks)[0]
    match = got['hota_frames']['match']
    for f, pairs in enumerate(ref['pairs']):
        assert {(a, int(d)) for a, d in enumerate(match[f]) if d >= 0} == pairs, f
    h = got['all']['hota']
    assert h['integers']['tp'] == ref['tp'] and ref['tp'][0] > 0
    for key, bound in (('deta', 1e-12), ('detre', 1e-12), ('detpr', 1e-12), ('assa', 2.0 ** -20), ('assre', 2.0 ** -20), ('asspr', 2.0 ** -20),
                       ('loca', 2.0 ** -20)):
        worst = max(abs(a - b) for a, b in zip(h['thresholds'][key], ref[key]))
        print(name, key, worst)
        assert worst <= bound, (key, worst)
    worst = max(abs(a * a - b * b) for a, b in zip(h['thresholds']['hota'], ref['hota']))
    print(name, 'hota^2', worst)
    assert worst <= 2.0 ** -19


# ---------------------------------------------------------------------------------------------------- the opt-in, errors, command lines
def test_without_hota_the_result_is_todays():
    labels, tracks = O.scene(21, frames=5, cars=5)
    plain, default = M.evaluate_sequences([labels], [tracks], hota=False), M.evaluate_sequences([labels], [tracks])
    with_hota = M.evaluate_sequences([labels], [tracks], hota=True)
    assert set(plain) == set(default) == {'params', 'names', 'sequences', 'all', 'trajectories', 'frames', 'seq_start'}
    assert set(with_hota) == set(plain) | {'hota_frames', 'hota_pairs'}
    assert plain['all'] == default['all'] and 'hota' not in plain['all'] and 'hota' not in plain['sequences'][0]
    assert {k: v for k, v in with_hota['all'].items() if k != 'hota'} == plain['all']
    assert {k: v for k, v in with_hota['sequences'][0].items() if k != 'hota'} == plain['sequences'][0]
    for key in plain['frames']:
        assert np.array_equal(plain['frames'][key], with_hota['frames'][key])
    assert M.summary_table(plain).startswith('CLEAR-MOT, Car, image overlap >= 0.5') and 'HOTA' not in M.summary_table(plain)
    assert set(M.result_as_json(plain)) == {'params', 'all', 'sequences', 'trajectories'}


def test_value_errors(monkeypatch):
    labels, tracks = O.scene(21, frames=5, cars=5)
    monkeypatch.setattr(PT, 'MAX_FRAMES', 4)
    with pytest.raises(ValueError, match='at most 4'):
        M.evaluate_sequences([labels], [tracks], hota=True)
    assert 'hota' not in M.evaluate_sequences([labels], [tracks])['all']                # (the limit is HOTA's alone)
    with pytest.raises(ValueError, match='at most 4'):
        PT.tables([0, 5], [3], [3])
    for bad in (dict(metric='iou'), dict(min_overlap=1.5)):
        with pytest.raises(ValueError):
            H.evaluate_hota_sequences([labels], [tracks], **bad)


def test_tables_geometry():
    seq_tab, frame_tab, cells, vecs = PT.tables([0, 2, 2, 5], [3, 0, 2], [4, 0, 5])
    assert seq_tab.tolist() == [[0, 3, 4, 0, 0, 2], [12, 0, 0, 7, 2, 2], [12, 2, 5, 7, 2, 5]] and (cells, vecs) == (22, 14)
    assert frame_tab.tolist() == [[0, 3, 4, 0]] * 2 + [[12, 2, 5, 7]] * 3
    rows = np.full((3, 2, 36), -1.0, np.float32)
    rows[0, :, 14] = rows[1, 0, 14] = rows[2, 1, 14] = 0.0
    trk, n_trk = PT.tracker_index_np(rows, np.array([[9, 4], [7, 4], [-1, 9]], np.int32), [0, 2, 3])
    assert trk.tolist() == [[2, 0], [1, -1], [-1, 0]] and n_trk == [3, 1] and trk.dtype == np.int32


def test_command_lines(tmp_path, capsys):
    from keras_retinanet_3D.bin import evaluate_tracking, run_network, track_results
    labels, tracks = O.scene(21, frames=5, cars=5)
    write_scene(tmp_path, '0000.txt', labels, tracks)
    write_scene(tmp_path, '0001.txt', *O.scene(22, frames=3, cars=4))
    direct = M.evaluate_sequences([labels], [tracks], hota=True)
    result = evaluate_tracking.main([str(tmp_path / 'label_02'), str(tmp_path / 'tracks'), '--hota', '--json', str(tmp_path / 'out.json')])
    assert result['sequences'][0]['hota'] == direct['all']['hota']
    text = capsys.readouterr().out.strip().splitlines()
    assert text[0] == 'CLEAR-MOT and HOTA, Car, image overlap >= 0.5' and len(text) == 5
    assert text[1].split()[-8:] == ['HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA']
    assert float(text[2].split()[-8]) == pytest.approx(100.0 * direct['all']['hota']['hota'], abs=0.005)
    saved = json.load(open(str(tmp_path / 'out.json')))
    assert saved['all']['hota'] == result['all']['hota'] and saved['sequences']['0000']['hota']['integers'] == direct['all']['hota']['integers']
    plain = evaluate_tracking.main([str(tmp_path / 'label_02'), str(tmp_path / 'tracks')])
    assert 'hota' not in plain['all'] and capsys.readouterr().out.startswith('CLEAR-MOT, Car')
    base = ['m.h5', 'img', 'calib', 'planes.mat', 'out']
    args = run_network.parse_args(base + ['--device-pose', '--track', 'dist', '--track-threshold', '2', '--tracking-labels', 'l.txt', '--hota'])
    assert args.hota and not run_network.parse_args(base).hota
    with pytest.raises(SystemExit):
        run_network.parse_args(base + ['--hota'])
    line = 'Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 {:.2f} 1.65 {:.2f} 0.00 {:.2f}\n'
    (tmp_path / 'r').mkdir()
    (tmp_path / 'r' / '000000.txt').write_text(line.format(1.0, 20.0, 0.9))
    (tmp_path / 'r' / '000001.txt').write_text(line.format(1.5, 20.5, 0.7))
    (tmp_path / 'l.txt').write_text(''.join('{} 4 Car 0 0 0.25 100 100 200 180 1.5 2 3 1 1.65 20 0\n'.format(k) for k in range(2)))
    result = track_results.main([str(tmp_path / 'r'), str(tmp_path / 't.txt'), '--metric', 'dist', '--threshold', '2', '--host',
                                 '--labels', str(tmp_path / 'l.txt'), '--hota'])
    assert result['all']['hota']['hota'] == 1.0 and result['all']['hota']['integers']['tp'] == [2] * 19
    assert 'CLEAR-MOT and HOTA' in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- header and ABI
def test_header_constants_and_contract():
    text = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    define = lambda name: int(re.search(r'#define {}\s+(\d+)'.format(name), text).group(1))  # noqa: E731
    assert define('GPP_HOTA_LEVELS') == H.LEVELS == hip.GPP_HOTA_LEVELS == HO.LEVELS == 19
    assert define('GPP_HOTA_HIST') == H.HIST == hip.GPP_HOTA_HIST == 20
    assert define('GPP_HOTA_FRAME_COLS') == H.FRAME_COLS == hip.GPP_HOTA_FRAME_COLS == 40
    assert define('GPP_HOTA_SEQ_COLS') == H.SEQ_COLS == hip.GPP_HOTA_SEQ_COLS == 8 and len(H.SEQ_INTEGERS) == 7
    assert define('GPP_HOTA_TAB_COLS') == hip.GPP_HOTA_TAB_COLS == 4 and define('GPP_HOTA_SEQ_TAB_COLS') == hip.GPP_HOTA_SEQ_TAB_COLS == 6
    assert H.SCALE == HO.S == 1 << define('GPP_MOT_SCALE_BITS') and PT.PAIR_TABLE_BYTES == 1 << 30 and PT.MAX_FRAMES == 1 << 20
    contract = ' '.join(text[text.index('HOTA scoring of tracks on the device'):text.index('#define GPP_HOTA_LEVELS')].replace('\n *', '\n').split())
    for phrase in ('UNPINNED', 'there is no admissibility test', 'operation for operation', 'on the HOST', 'ZEROED by the caller',
                   'EVERY frame of a sequence before gpp_hota_match', 'GPP_ERR_UNSUPPORTED', 'GPP_ERR_WORKSPACE', '(20 q + 19) >> 20'):
        assert phrase in contract, phrase
    makefile = open(os.path.join(ROOT, 'ground-plane-polling_amd', 'csrc', 'Makefile')).read()
    assert 'hota_eval.hip' in re.search(r'SRCS_EXACT = (.*)', makefile).group(1) and '$(OBJ)/hota_eval.o: hota_eval.hip mot_assign.h' in makefile


def tab(lines):
    flat = [v for line in lines for v in line]
    return (ctypes.c_int32 * max(len(flat), 1))(*flat)


GOOD = [[0, 2, 3, 0]] * 4                       # four frames of one sequence: 6 cells, 5 counters
FRAME_CALLS = [('n_negative', -1, 4, 4, 0, GOOD, 6, 5, -1), ('d_negative', 4, -1, 4, 0, GOOD, 6, 5, -1), ('a_negative', 4, 4, -1, 0, GOOD, 6, 5, -1),
               ('cells_negative', 4, 4, 4, 0, GOOD, -1, 5, -1), ('vecs_negative', 4, 4, 4, 0, GOOD, 6, -1, -1),
               ('metric_3', 4, 4, 4, 3, GOOD, 6, 5, -1), ('metric_negative', 4, 4, 4, -1, GOOD, 6, 5, -1),
               ('d_129', 4, 129, 4, 0, GOOD, 6, 5, -4), ('a_129', 4, 4, 129, 0, GOOD, 6, 5, -4), ('cells_2_31', 4, 4, 4, 0, GOOD, 1 << 31, 5, -4),
               ('nothing_to_do', 0, 4, 4, 0, GOOD, 6, 5, 0), ('null_pointers', 4, 4, 4, 0, GOOD, 6, 5, -1)]
# with every pointer in place (host memory: a refusal returns before anything is launched or copied)
TABLE_CALLS = [('cells_outside', [[0, 2, 3, 0]] * 3 + [[1, 2, 3, 0]], 6, 5, -1), ('counters_outside', [[0, 2, 3, 1]] * 4, 6, 5, -1),
               ('base_descending', [[6, 2, 3, 5]] * 2 + [[0, 2, 3, 0]] * 2, 12, 10, -1), ('vec_base_descending', [[0, 2, 3, 5], [0, 2, 3, 0]] * 2, 12, 10, -1),
               ('negative_entry', [[0, -2, 3, 0]] * 4, 6, 5, -1), ('negative_base', [[-1, 2, 3, 0]] * 4, 6, 5, -1),
               ('short_workspace', GOOD, 6, 5, -2)]


@pytest.mark.parametrize('what,N,D,A,metric,lines,cells,vecs,code', FRAME_CALLS, ids=[c[0] for c in FRAME_CALLS])
def test_potential_and_match_refuse_before_any_launch(what, N, D, A, metric, lines, cells, vecs, code):
    """ host code: every device pointer is null -- a refusal returns before it is looked at """
    lib = hip.lib()
    assert lib.gpp_hota_potential(None, None, None, None, None, N, D, A, metric, tab(lines), cells, vecs, None, 0, None) == code
    assert lib.gpp_hota_match(None, None, None, None, None, N, D, A, metric, tab(lines), cells, vecs, None, None, None, 0, None) == code


@pytest.mark.parametrize('what,lines,cells,vecs,code', TABLE_CALLS, ids=[c[0] for c in TABLE_CALLS])
def test_tables_are_checked_before_any_launch(what, lines, cells, vecs, code):
    lib = hip.lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    short = 64                                  # bytes: below any table
    size = short if what == 'short_workspace' else 2048
    assert lib.gpp_hota_potential(p, p, p, p, p, 4, 4, 4, 0, tab(lines), cells, vecs, p, size, None) == code
    assert lib.gpp_hota_match(p, p, p, p, p, 4, 4, 4, 0, tab(lines), cells, vecs, p, p, p, size, None) == code
    if what == 'short_workspace':
        assert lib.gpp_hota_potential(p, p, p, p, p, 4, 4, 4, 0, tab(lines), cells, vecs, ctypes.c_void_p(base + 4), 2048, None) == -3


REDUCE_CALLS = [('n_negative', -1, [[0, 2, 3, 0, 0, 0]], 6, 5, -1), ('cells_negative', 4, [[0, 2, 3, 0, 0, 4]], -1, 5, -1),
                ('frames_beyond', 4, [[0, 2, 3, 0, 0, 5]], 6, 5, -1), ('frames_descending', 4, [[0, 2, 3, 0, 3, 2]], 6, 5, -1),
                ('frames_overlap', 4, [[0, 2, 3, 0, 0, 3], [6, 1, 1, 5, 2, 4]], 7, 7, -1), ('cells_outside', 4, [[1, 2, 3, 0, 0, 4]], 6, 5, -1),
                ('base_descending', 4, [[6, 2, 3, 5, 0, 2], [0, 2, 3, 0, 2, 4]], 12, 10, -1), ('cells_2_31', 4, [[0, 2, 3, 0, 0, 4]], 1 << 31, 5, -4),
                ('short_workspace', 4, [[0, 2, 3, 0, 0, 4]], 6, 5, -2), ('no_sequence', 4, [], 6, 5, 0)]


@pytest.mark.parametrize('what,N,lines,cells,vecs,code', REDUCE_CALLS, ids=[c[0] for c in REDUCE_CALLS])
def test_reduce_refuses_before_any_launch(what, N, lines, cells, vecs, code):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    assert hip.lib().gpp_hota_reduce(p, N, tab(lines), len(lines), cells, vecs, p, p, 64 if what == 'short_workspace' else 2048, None) == code
    if what == 'short_workspace':
        assert hip.lib().gpp_hota_reduce(None, N, tab(lines), len(lines), cells, vecs, None, None, 2048, None) == -1     # null pointers


def test_workspace_sizes():
    n = ctypes.c_size_t(0)
    assert hip.hota_workspace_bytes(0, 0, 0, 0) == 0 and hip.hota_workspace_bytes(6, 5, 4, 1) == 768
    # P 48 bytes, A 24, hist at 80 (72 rounded up to 16) 480, counters at 560 20, the table at 592: 4 frames of 16 bytes beat 1 sequence of 24
    assert hip.hota_workspace_bytes(6, 5, 0, 1) == 768 and hip.hota_workspace_bytes(6, 5, 11, 1) == 768 and hip.hota_workspace_bytes(6, 5, 12, 1) == 1024
    assert hip.lib().gpp_hota_workspace_bytes(-1, 0, 0, 0, ctypes.byref(n)) == -1 and hip.lib().gpp_hota_workspace_bytes(1, 1, 1, 1, None) == -1
    assert hip.lib().gpp_hota_workspace_bytes(1 << 31, 0, 0, 0, ctypes.byref(n)) == -4
