""" CPU tests of the identity scores: the NumPy form (utils/idf1_eval.py) against the loop-written oracle
(tests/idf1_oracle.py) and against the metric's definition ((G + T)^2 matrix, scipy); hand-derived cases; the opt-in leaves today's result
alone; the ValueErrors; the command lines; the C ABI's argument checks (host code: they come before any launch). """
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import hota_oracle as HO
import idf1_oracle as IO
import mot_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import idf1_eval as I
from keras_retinanet_3D.utils import mot_eval as M
from keras_retinanet_3D.utils import pair_tables as PT
from test_mot_eval_cpu import write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = O.named_cases()
S = 1 << 20
SCENES = dict([(name, (CASES[name][0], CASES[name][1], CASES[name][3])) for name in sorted(CASES)] +
              [('split', HO.split_case() + ({},)), ('tie', HO.tie_case() + ({},)), ('dense_sequence', HO.dense_sequence() + ({},))])
SEEDED = [('scene_{}_{}'.format(seed, k), O.scene(seed, **kw)) for k, (seed, kw) in enumerate(HO.SCENES)]
_RESULTS = {}


def scored(name):
    """ (the NumPy form's result, the oracle's), computed once per scene """
    if name not in _RESULTS:
        labels, tracks, options = SCENES[name]
        _RESULTS[name] = (M.evaluate_sequences(labels, tracks, idf1=True, **options), IO.evaluate(labels, tracks, **options))
    return _RESULTS[name]


def same_as_oracle(got, want, labels, tracks):
    assert len(got['idf1_pairs']) == len(want) == len(got['sequences'])
    for s, (w, (cars, live)) in enumerate(zip(want, IO.sequence_ids(labels, tracks))):
        pairs = got['idf1_pairs'][s]
        assert got['trajectories'][s]['track_ids'].tolist() == cars
        assert all(pairs[key].dtype == np.int32 for key in ('C', 'gc', 'tc', 'match'))
        assert pairs['C'].shape == (len(cars), len(live)) == (w['G'], w['T'])
        assert pairs['gc'].shape == (len(cars),) and pairs['tc'].shape == (len(live),) and pairs['match'].shape == (len(cars),)
        C = {(cars[g], live[t]): int(pairs['C'][g, t]) for g in range(len(cars)) for t in range(len(live)) if pairs['C'][g, t]}
        assert C == w['C']
        assert {g: int(n) for g, n in zip(cars, pairs['gc']) if n} == w['gc'] and {t: int(n) for t, n in zip(live, pairs['tc']) if n} == w['tc']
        assert {g: (live[m] if m >= 0 else None) for g, m in zip(cars, pairs['match'])} == w['match']
        assert got['sequences'][s]['idf1']['integers'] == {'idtp': w['idtp'], 'idfn': w['idfn'], 'idfp': w['idfp']}
    assert got['all']['idf1']['integers'] == {key: sum(w[key] for w in want) for key in ('idtp', 'idfn', 'idfp')}


# ---------------------------------------------------------------------------------------------------- the oracle and the definition
@pytest.mark.parametrize('name', sorted(SCENES))
def test_numpy_form_equals_the_oracle(name):
    labels, tracks, _ = SCENES[name]
    got, want = scored(name)
    same_as_oracle(got, want, labels, tracks)


@pytest.mark.parametrize('name', sorted(SCENES))
def test_integers_equal_the_definition(name):
    labels, tracks, options = SCENES[name]
    got, _ = scored(name)
    for e, ref in zip(got['sequences'], IO.float_identity(labels, tracks, **options)):
        assert (e['idf1']['integers']['idtp'], e['idf1']['integers']['idfn'], e['idf1']['integers']['idfp']) == ref


@pytest.mark.parametrize('name', [n for n, _ in SEEDED])
def test_seeded_scenes_equal_the_oracle_and_the_definition(name):
    labels, tracks = dict(SEEDED)[name]
    got = I.evaluate_idf1_sequences([labels], [tracks])
    same_as_oracle(got, IO.evaluate([labels], [tracks]), [labels], [tracks])
    ints = got['all']['idf1']['integers']
    assert (ints['idtp'], ints['idfn'], ints['idfp']) == IO.float_identity([labels], [tracks])[0] and ints['idtp'] > 0
    assert 0.0 < got['all']['idf1']['idf1'] < 1.0


@pytest.mark.parametrize('metric', ['bev', '3d'])
def test_other_metrics_equal_the_oracle(metric):
    labels, tracks = O.scene(7, frames=4, cars=6)
    got = I.evaluate_idf1_sequences([labels], [tracks], metric=metric, min_overlap=0.25)
    same_as_oracle(got, IO.evaluate([labels], [tracks], metric=metric, min_overlap=0.25), [labels], [tracks])
    assert got['all']['idf1']['integers']['idtp'] > 0


@pytest.mark.parametrize('G,T', [(3, 7), (5, 5), (8, 2), (1, 1), (6, 8)])
def test_random_tables_equal_the_oracle_and_the_definition(G, T):
    """ 200 small tables with ties and zero cells, G < T, G = T and G > T: the rectangular form against the loops, its IDFN / IDFP against
    the (G + T)^2 formulation, its total against scipy's on the same rectangular matrix """
    for seed in range(40):
        rng = np.random.default_rng(1000 * G + 10 * T + seed)
        C = (rng.integers(0, 4, (G, T)) * (rng.random((G, T)) < 0.6)).astype(np.int32)
        gc, tc = (C.sum(axis=1) + rng.integers(0, 3, G)).astype(np.int32), (C.sum(axis=0) + rng.integers(0, 3, T)).astype(np.int32)
        match, line = I.seq_counts_np(C, gc, tc)
        want, idtp, cost = IO.table_scores({(g, t): int(C[g, t]) for g in range(G) for t in range(T)}, G, T)
        assert match.tolist() == want and match.dtype == np.int32
        assert line.tolist() == [idtp, int(gc.sum()) - idtp, int(tc.sum()) - idtp, int(gc.sum()), int(tc.sum()), cost, G, T]
        assert tuple(line[:3]) == IO.definition_counts(C, gc, tc) and cost == IO.rectangular_total(C), seed


def test_several_sequences_sum():
    scenes = [O.scene(41, frames=17, cars=9, quantum=16.0), (([], []), ([], [])), O.scene(42, frames=5, cars=20), O.dense(3, 30, 40)]
    labels, tracks = [s[0] for s in scenes], [s[1] for s in scenes]
    got = I.evaluate_idf1_sequences(labels, tracks)
    same_as_oracle(got, IO.evaluate(labels, tracks), labels, tracks)
    assert all(got['sequences'][1]['idf1'][key] is None for key in I.RATIOS) and got['all']['idf1']['idf1'] > 0
    assert got['idf1_pairs'][1]['C'].shape == (0, 0) and got['idf1_pairs'][3]['C'].shape == (30, 40)


# ---------------------------------------------------------------------------------------------------- hand-derived cases
def test_perfect():
    got, _ = scored('perfect')
    assert got['all']['idf1'] == {'idf1': 1.0, 'idr': 1.0, 'idp': 1.0, 'integers': {'idtp': 10, 'idfn': 0, 'idfp': 0}}
    assert got['idf1_pairs'][0]['C'].tolist() == [[5, 0], [0, 5]] and got['idf1_pairs'][0]['match'].tolist() == [0, 1]


def test_split():
    """ one car under id 7 and then id 9, three frames each: one id explains half the frames, the other is charged in full """
    labels, tracks = HO.split_case()
    got = M.evaluate_sequences(labels, tracks, hota=True, idf1=True)
    e = got['all']['idf1']
    assert e['integers'] == {'idtp': 3, 'idfn': 3, 'idfp': 3} and e['idf1'] == e['idr'] == e['idp'] == 0.5
    assert got['idf1_pairs'][0]['C'].tolist() == [[3, 3]] and got['idf1_pairs'][0]['match'].tolist() == [0]      # (the first of two equals)
    assert got['all']['hota']['thresholds']['hota'] == [math.sqrt(0.5)] * 19 and got['all']['mota'] == 1.0 - 1.0 / 6.0


def test_swap():
    """ two cars whose ids change hands after frame 3 of 5: each keeps the id it had for three frames """
    got, _ = scored('swap')
    assert got['idf1_pairs'][0]['C'].tolist() == [[3, 2], [2, 3]] and got['all']['idf1']['integers'] == {'idtp': 6, 'idfn': 4, 'idfp': 4}
    assert got['all']['idf1']['idf1'] == 0.6


def test_an_overlap_of_exactly_one_half_counts_and_the_double_below_does_not():
    got, _ = scored('threshold')                         # frame 0: 64 / 128; frame 1: 64 / (128 + 2^-12)
    assert got['idf1_pairs'][0]['C'].tolist() == [[1]] and got['idf1_pairs'][0]['gc'].tolist() == [2] and got['idf1_pairs'][0]['tc'].tolist() == [2]
    assert got['all']['idf1']['integers'] == {'idtp': 1, 'idfn': 1, 'idfp': 1}
    C, gc, tc = np.zeros((1, 1), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    below = np.nextafter(0.5, 0.0)
    for o, want in ((0.5, 1), (below, 1), (1.0, 2), (float('nan'), 2), (0.0, 2)):
        q, gl, rl = PT.similarity_np(np.array([[o]]), [1], [3])
        I.count_np(q, [0], [0], C, gc, tc)
        assert int(C[0, 0]) == want, o
    assert gc.tolist() == [5] and tc.tolist() == [5] and int(np.floor(below * S)) == (S >> 1) - 1


def test_one_label_counts_with_two_rows_of_a_frame():
    """ the tie case's last frame holds two identical rows, ids 9 and 7: the label counts with both -- no one-to-one rule inside a frame """
    got, _ = scored('tie')
    pairs = got['idf1_pairs'][0]
    assert pairs['C'].tolist() == [[4, 1]] and pairs['gc'].tolist() == [4] and pairs['tc'].tolist() == [4, 1] and pairs['C'].sum() > pairs['gc'].sum()
    assert got['all']['idf1']['integers'] == {'idtp': 4, 'idfn': 0, 'idfp': 1}
    assert got['all']['idf1']['idr'] == 1.0 and got['all']['idf1']['idp'] == 0.8 and got['all']['idf1']['idf1'] == 8.0 / 9.0


def test_counters_equal_hotas_when_both_are_requested():
    for labels, tracks in ([dict(SEEDED)['scene_31_0'][0]], [dict(SEEDED)['scene_31_0'][1]]), HO.dense_sequence():
        got = M.evaluate_sequences(labels, tracks, hota=True, idf1=True)
        for a, b in zip(got['idf1_pairs'], got['hota_pairs']):
            assert np.array_equal(a['gc'], b['gc']) and np.array_equal(a['tc'], b['tc']) and a['gc'].dtype == b['gc'].dtype
            assert a['C'].shape == b['P'].shape and not (a['C'] > 0)[b['P'] == 0].any()     # (no overlap, no count)


def same_tree(a, b):
    """ two results, key for key: arrays by dtype, shape and value, everything else by == """
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def test_the_host_form_computes_a_frames_overlaps_once(monkeypatch):
    """ with both scores requested the NumPy form walks every frame's overlaps once -- the assignment, HOTA and the identity scores work on
    the same ones -- and the result is what it is without the counter """
    labels, tracks, _, options = CASES['empty']          # two sequences, of three frames and of none
    frames = sum(max(len(g[0]), len(t[0])) for g, t in zip(labels, tracks))
    assert len(labels) == 2 and frames == 3
    want = M.evaluate_sequences(labels, tracks, device=False, hota=True, idf1=True, **options)
    calls = []
    monkeypatch.setattr(M.kitti_eval, 'image_overlaps', lambda *a, _f=M.kitti_eval.image_overlaps: calls.append(1) or _f(*a))
    got = M.evaluate_sequences(labels, tracks, device=False, hota=True, idf1=True, **options)
    assert len(calls) == frames
    assert {'hota_frames', 'hota_pairs', 'idf1_pairs'} <= set(got) and same_tree(got, want)


def test_ignored_and_empty():
    got, _ = scored('ignored')
    assert got['all']['idf1'] == {'idf1': None, 'idr': None, 'idp': None, 'integers': {'idtp': 0, 'idfn': 0, 'idfp': 0}}
    got, _ = scored('empty')                             # sequence 0: a lone row and a lone label; sequence 1: no frames
    assert all(got['sequences'][1]['idf1'][name] is None for name in I.RATIOS)
    assert got['sequences'][0]['idf1'] == {'idf1': 0.0, 'idr': 0.0, 'idp': 0.0, 'integers': {'idtp': 0, 'idfn': 1, 'idfp': 1}}
    assert got['idf1_pairs'][0]['match'].tolist() == [-1]
    none = I.evaluate_idf1_sequences([], [])
    assert all(none['all']['idf1'][name] is None for name in I.RATIOS) and none['idf1_pairs'] == []


def test_a_trajectory_paired_with_an_id_it_never_met_reports_none():
    match, idtp, cost = I.assign_table_np(np.array([[0, 0, 0], [0, 2, 0]], np.int32))
    assert match.tolist() == [-1, 1] and idtp == 2 and cost == 2 * S - 2
    match, idtp, cost = I.assign_table_np(np.zeros((3, 2), np.int32))
    assert match.tolist() == [-1, -1, -1] and idtp == 0 and cost == 3 * S
    assert I.assign_table_np(np.zeros((0, 5), np.int32))[1:] == (0, 0) and I.assign_table_np(np.zeros((4, 0), np.int32))[0].tolist() == [-1] * 4


def test_the_sparse_table_at_the_limits_is_quick_on_the_host():
    """ the generator's parameters of the GPU test's largest table: the NumPy form alone must stay within seconds """
    import time
    C = IO.cap_table()
    t0 = time.perf_counter()
    match, idtp, cost = I.assign_table_np(C)
    seconds = time.perf_counter() - t0
    print('1024 x 4096, four cells a row in the first 1024 columns: {:.2f} s'.format(seconds))                  # (1.6 s where it was written)
    assert C.shape == (1024, 4096) and cost == IO.rectangular_total(C) and idtp > 0 and (C > 0).sum(axis=1).max() <= 4
    assert (match >= 0).sum() < 1024                     # (the trajectories compete: some end on an id they never met)


# ---------------------------------------------------------------------------------------------------- the opt-in, errors, command lines
def test_without_idf1_the_result_is_todays():
    labels, tracks = O.scene(21, frames=5, cars=5)
    plain, default = M.evaluate_sequences([labels], [tracks], idf1=False), M.evaluate_sequences([labels], [tracks])
    assert set(plain) == set(default) == {'params', 'names', 'sequences', 'all', 'trajectories', 'frames', 'seq_start'}
    assert plain['all'] == default['all'] and 'idf1' not in plain['all'] and 'idf1' not in plain['sequences'][0]
    with_idf1 = M.evaluate_sequences([labels], [tracks], idf1=True)
    assert set(with_idf1) == set(plain) | {'idf1_pairs'}
    assert {k: v for k, v in with_idf1['all'].items() if k != 'idf1'} == plain['all']
    assert {k: v for k, v in with_idf1['sequences'][0].items() if k != 'idf1'} == plain['sequences'][0]
    for key in plain['frames']:
        assert np.array_equal(plain['frames'][key], with_idf1['frames'][key])
    hota, both = M.evaluate_sequences([labels], [tracks], hota=True, idf1=False), M.evaluate_sequences([labels], [tracks], hota=True, idf1=True)
    assert set(hota) == set(plain) | {'hota_frames', 'hota_pairs'} and set(both) == set(hota) | {'idf1_pairs'}
    assert hota['all'] == {k: v for k, v in both['all'].items() if k != 'idf1'} and both['all']['idf1'] == with_idf1['all']['idf1']
    assert M.summary_table(plain).startswith('CLEAR-MOT, Car, image overlap >= 0.5') and 'IDF1' not in M.summary_table(plain)
    assert M.summary_table(hota).startswith('CLEAR-MOT and HOTA, Car') and 'IDF1' not in M.summary_table(hota)
    assert set(M.result_as_json(plain)) == {'params', 'all', 'sequences', 'trajectories'}
    json.dumps(M.result_as_json(both))


def test_value_errors(monkeypatch):
    with pytest.raises(ValueError, match='at most 1024'):
        I.assign_table_np(np.zeros((1025, 1), np.int32))
    with pytest.raises(ValueError, match='at most 4096'):
        I.assign_table_np(np.zeros((1, 4097), np.int32))
    I.check_sides(1024, 4096)
    labels, tracks = O.scene(21, frames=5, cars=5)
    monkeypatch.setattr(I, 'MAX_IDS', 3)
    with pytest.raises(ValueError, match='at most 3'):
        M.evaluate_sequences([labels], [tracks], idf1=True)
    assert 'idf1' not in M.evaluate_sequences([labels], [tracks])['all']                # (the limit is IDF1's alone)
    monkeypatch.setattr(I, 'MAX_IDS', 4096)
    monkeypatch.setattr(I, 'MAX_TRAJECTORIES', 2)
    with pytest.raises(ValueError, match='at most 2'):
        M.evaluate_sequences([labels], [tracks], idf1=True)
    monkeypatch.setattr(I, 'MAX_TRAJECTORIES', 1024)
    monkeypatch.setattr(PT, 'MAX_FRAMES', 4)
    with pytest.raises(ValueError, match='at most 4'):
        M.evaluate_sequences([labels], [tracks], idf1=True)
    for bad in (dict(metric='iou'), dict(min_overlap=1.5)):
        with pytest.raises(ValueError):
            I.evaluate_idf1_sequences([labels], [tracks], **bad)


def test_summary():
    assert I.summarise_idf1([3, 1, 2]) == {'idf1': 6.0 / 9.0, 'idr': 0.75, 'idp': 0.6, 'integers': {'idtp': 3, 'idfn': 1, 'idfp': 2}}
    assert I.summarise_idf1([0, 0, 5])['idr'] == 0.0 and I.summarise_idf1([0, 0, 5])['idf1'] == 0.0
    assert I.summarise_idf1(np.array([0, 0, 0, 0, 0, 0, 4, 4]))['idf1'] is None
    assert all(type(v) is int for v in I.summarise_idf1(np.array([3, 1, 2], np.int64))['integers'].values())


def test_command_lines(tmp_path, capsys):
    from keras_retinanet_3D.bin import evaluate_tracking, run_network, track_results
    labels, tracks = O.scene(21, frames=5, cars=5)
    write_scene(tmp_path, '0000.txt', labels, tracks)
    write_scene(tmp_path, '0001.txt', *O.scene(22, frames=3, cars=4))
    direct = M.evaluate_sequences([labels], [tracks], idf1=True)
    result = evaluate_tracking.main([str(tmp_path / 'label_02'), str(tmp_path / 'tracks'), '--idf1', '--json', str(tmp_path / 'out.json')])
    assert result['sequences'][0]['idf1'] == direct['all']['idf1']
    text = capsys.readouterr().out.strip().splitlines()
    assert text[0] == 'CLEAR-MOT and Identity, Car, image overlap >= 0.5' and len(text) == 5
    assert text[1].split()[-3:] == ['IDF1', 'IDR', 'IDP']
    assert [float(v) for v in text[2].split()[-3:]] == pytest.approx([100.0 * direct['all']['idf1'][k] for k in I.RATIOS], abs=0.005)
    saved = json.load(open(str(tmp_path / 'out.json')))
    assert saved['all']['idf1'] == result['all']['idf1'] and saved['sequences']['0000']['idf1']['integers'] == direct['all']['idf1']['integers']
    result = evaluate_tracking.main([str(tmp_path / 'label_02'), str(tmp_path / 'tracks'), '--hota', '--idf1'])
    text = capsys.readouterr().out.strip().splitlines()
    assert text[0] == 'CLEAR-MOT, HOTA and Identity, Car, image overlap >= 0.5'
    assert text[1].split()[-11:] == ['HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA', 'IDF1', 'IDR', 'IDP']
    assert len(text[2].split()) == len(text[1].split()) and 'hota' in result['all'] and 'idf1' in result['all']
    with_flag_off = evaluate_tracking.main([str(tmp_path / 'label_02'), str(tmp_path / 'tracks')])
    out = capsys.readouterr().out
    assert 'idf1' not in with_flag_off['all'] and out == M.summary_table(M.evaluate_tracking(str(tmp_path / 'label_02'), str(tmp_path / 'tracks'))) + '\n'
    assert out.startswith('CLEAR-MOT, Car') and 'IDF1' not in out
    base = ['m.h5', 'img', 'calib', 'planes.mat', 'out']
    args = run_network.parse_args(base + ['--device-pose', '--track', 'dist', '--track-threshold', '2', '--tracking-labels', 'l.txt', '--idf1'])
    assert args.idf1 and not args.hota and not run_network.parse_args(base).idf1
    with pytest.raises(SystemExit):
        run_network.parse_args(base + ['--idf1'])
    line = 'Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 {:.2f} 1.65 {:.2f} 0.00 {:.2f}\n'
    (tmp_path / 'r').mkdir()
    (tmp_path / 'r' / '000000.txt').write_text(line.format(1.0, 20.0, 0.9))
    (tmp_path / 'r' / '000001.txt').write_text(line.format(1.5, 20.5, 0.7))
    (tmp_path / 'l.txt').write_text(''.join('{} 4 Car 0 0 0.25 100 100 200 180 1.5 2 3 1 1.65 20 0\n'.format(k) for k in range(2)))
    result = track_results.main([str(tmp_path / 'r'), str(tmp_path / 't.txt'), '--metric', 'dist', '--threshold', '2', '--host',
                                 '--labels', str(tmp_path / 'l.txt'), '--idf1'])
    assert result['all']['idf1']['idf1'] == 1.0 and result['all']['idf1']['integers'] == {'idtp': 2, 'idfn': 0, 'idfp': 0}
    assert 'CLEAR-MOT and Identity' in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- header and ABI
def test_header_constants_and_contract():
    text = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    define = lambda name: int(re.search(r'#define {}\s+(\d+)'.format(name), text).group(1))  # noqa: E731
    assert define('GPP_IDF1_MAX_IDS') == I.MAX_IDS == hip.GPP_IDF1_MAX_IDS == 4096
    assert define('GPP_IDF1_SEQ_COLS') == I.SEQ_COLS == hip.GPP_IDF1_SEQ_COLS == 8
    assert define('GPP_MOT_MAX_TRAJECTORIES') == I.MAX_TRAJECTORIES == 1024 and I.SCALE == IO.S == 1 << define('GPP_MOT_SCALE_BITS')
    assert I.HALF == IO.HALF == S >> 1
    contract = ' '.join(text[text.index('Identity scoring of tracks on the device'):text.index('#define GPP_IDF1_MAX_IDS')].replace('\n *', '\n').split())
    for phrase in ('UNPINNED', 'operation for operation', 'on the HOST', 'ZEROED by the caller', 'read AND WRITE', 'q(a, d) >= 2^19',
                   'EVERY frame of a sequence before gpp_idf1_assign', 'GPP_ERR_UNSUPPORTED', 'GPP_ERR_WORKSPACE', 'minv << 13 | column'):
        assert phrase in contract, phrase
    makefile = open(os.path.join(ROOT, 'ground-plane-polling_amd', 'csrc', 'Makefile')).read()
    assert 'idf1_eval.hip' in re.search(r'SRCS_EXACT = (.*)', makefile).group(1) and '$(OBJ)/idf1_eval.o: idf1_eval.hip mot_assign.h' in makefile


def tab(lines):
    flat = [v for line in lines for v in line]
    return (ctypes.c_int32 * max(len(flat), 1))(*flat)


GOOD = [[0, 2, 3, 0]] * 4                       # four frames of one sequence: 6 cells, 5 counters
COUNT_CALLS = [('n_negative', -1, 4, 4, 0, GOOD, 6, 5, -1), ('d_negative', 4, -1, 4, 0, GOOD, 6, 5, -1), ('a_negative', 4, 4, -1, 0, GOOD, 6, 5, -1),
               ('cells_negative', 4, 4, 4, 0, GOOD, -1, 5, -1), ('vecs_negative', 4, 4, 4, 0, GOOD, 6, -1, -1),
               ('metric_3', 4, 4, 4, 3, GOOD, 6, 5, -1), ('metric_negative', 4, 4, 4, -1, GOOD, 6, 5, -1),
               ('d_129', 4, 129, 4, 0, GOOD, 6, 5, -4), ('a_129', 4, 4, 129, 0, GOOD, 6, 5, -4), ('cells_2_31', 4, 4, 4, 0, GOOD, 1 << 31, 5, -4),
               ('nothing_to_do', 0, 4, 4, 0, GOOD, 6, 5, 0), ('null_pointers', 4, 4, 4, 0, GOOD, 6, 5, -1)]
# with every pointer in place (host memory: a refusal returns before anything is launched or copied)
TABLE_CALLS = [('cells_outside', [[0, 2, 3, 0]] * 3 + [[1, 2, 3, 0]], 6, 5, -1), ('counters_outside', [[0, 2, 3, 1]] * 4, 6, 5, -1),
               ('base_descending', [[6, 2, 3, 5]] * 2 + [[0, 2, 3, 0]] * 2, 12, 10, -1), ('vec_base_descending', [[0, 2, 3, 5], [0, 2, 3, 0]] * 2, 12, 10, -1),
               ('negative_entry', [[0, -2, 3, 0]] * 4, 6, 5, -1), ('negative_base', [[-1, 2, 3, 0]] * 4, 6, 5, -1),
               ('short_workspace', GOOD, 6, 5, -2)]
ASSIGN_CALLS = [('s_negative', -1, [[0, 2, 3, 0, 0, 4]], 6, 5, -1), ('cells_negative', 1, [[0, 2, 3, 0, 0, 4]], -1, 5, -1),
                ('cells_outside', 1, [[1, 2, 3, 0, 0, 4]], 6, 5, -1), ('counters_outside', 1, [[0, 2, 3, 1, 0, 4]], 6, 5, -1),
                ('base_descending', 2, [[6, 2, 3, 5, 0, 2], [0, 2, 3, 0, 2, 4]], 12, 10, -1), ('negative_entry', 1, [[0, 2, -3, 0, 0, 4]], 6, 5, -1),
                ('cells_2_31', 1, [[0, 2, 3, 0, 0, 4]], 1 << 31, 5, -4), ('rows_1025', 1, [[0, 1025, 1, 0, 0, 4]], 1025, 1026, -4),
                ('ids_4097', 1, [[0, 1, 4097, 0, 0, 4]], 4097, 4098, -4), ('short_workspace', 1, [[0, 2, 3, 0, 0, 4]], 6, 5, -2),
                ('no_sequence', 0, [], 6, 5, 0)]


@pytest.mark.parametrize('what,N,D,A,metric,lines,cells,vecs,code', COUNT_CALLS, ids=[c[0] for c in COUNT_CALLS])
def test_count_refuses_before_any_launch(what, N, D, A, metric, lines, cells, vecs, code):
    """ host code: every device pointer is null -- a refusal returns before it is looked at """
    assert hip.lib().gpp_idf1_count(None, None, None, None, None, N, D, A, metric, tab(lines), cells, vecs, None, 0, None) == code


@pytest.mark.parametrize('what,lines,cells,vecs,code', TABLE_CALLS, ids=[c[0] for c in TABLE_CALLS])
def test_frame_tables_are_checked_before_any_launch(what, lines, cells, vecs, code):
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    size = 64 if what == 'short_workspace' else 2048
    assert hip.lib().gpp_idf1_count(p, p, p, p, p, 4, 4, 4, 0, tab(lines), cells, vecs, p, size, None) == code
    if what == 'short_workspace':
        assert hip.lib().gpp_idf1_count(p, p, p, p, p, 4, 4, 4, 0, tab(lines), cells, vecs, ctypes.c_void_p(base + 4), 2048, None) == -3


@pytest.mark.parametrize('what,S_,lines,cells,vecs,code', ASSIGN_CALLS, ids=[c[0] for c in ASSIGN_CALLS])
def test_assign_refuses_before_any_launch(what, S_, lines, cells, vecs, code):
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    assert hip.lib().gpp_idf1_assign(tab(lines), S_, cells, vecs, p, p, p, 16 if what == 'short_workspace' else 1 << 20, None) == code
    if what == 'short_workspace':
        assert hip.lib().gpp_idf1_assign(tab(lines), S_, cells, vecs, None, None, None, 2048, None) == -1                  # null pointers
        assert hip.lib().gpp_idf1_assign(tab(lines), S_, cells, vecs, p, p, ctypes.c_void_p(base + 4), 2048, None) == -3   # alignment


def test_workspace_sizes():
    n = ctypes.c_size_t(0)
    assert hip.idf1_workspace_bytes(0, 0, 0, 0) == 0 and hip.idf1_workspace_bytes(6, 5, 4, 1) == 256
    # C 24 bytes, the counters at 32 (24 rounded up to 16) 20, the table at 64: 12 frames of 16 bytes fill 256, 13 do not
    assert hip.idf1_workspace_bytes(6, 5, 12, 1) == 256 and hip.idf1_workspace_bytes(6, 5, 13, 1) == 512
    assert hip.idf1_workspace_bytes(6, 5, 0, 8) == 256 and hip.idf1_workspace_bytes(6, 5, 0, 9) == 512
    assert hip.lib().gpp_idf1_workspace_bytes(-1, 0, 0, 0, ctypes.byref(n)) == -1 and hip.lib().gpp_idf1_workspace_bytes(1, 1, 1, 1, None) == -1
    assert hip.lib().gpp_idf1_workspace_bytes(1 << 31, 0, 0, 0, ctypes.byref(n)) == -4
