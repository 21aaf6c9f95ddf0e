""" GPU tests of the identity scores: csrc/idf1_eval.hip against the NumPy form (utils/idf1_eval.py), which
tests/test_idf1_cpu.py holds against the loop-written oracle and the metric's definition -- equality of every array (with its dtype and
shape) and every integer; the assignment also directly through the C ABI, on tables written into the workspace. """
import ctypes

import numpy as np
import pytest
import torch

import hota_oracle as HO
import idf1_oracle as IO
import mot_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import idf1_eval as I
from keras_retinanet_3D.utils import kitti_eval
from keras_retinanet_3D.utils import mot_eval as M
from keras_retinanet_3D.utils import pair_tables as PT
from keras_retinanet_3D.utils import track as T
from test_hota_gpu import same_hota
from test_mot_eval_gpu import drive, same_result

pytestmark = pytest.mark.gpu

CASES = O.named_cases()
SCENES = {'split': HO.split_case, 'tie': HO.tie_case, 'dense_sequence': HO.dense_sequence}
S = 1 << 20


def same_idf1(got, want):
    same_result(got, want)                                                              # (everything of section 4.29, 'idf1' in the summaries included)
    assert set(got) == set(want) and len(got['idf1_pairs']) == len(want['idf1_pairs'])
    for a, b in zip(got['idf1_pairs'], want['idf1_pairs']):
        for key in ('C', 'gc', 'tc', 'match'):
            assert a[key].dtype == b[key].dtype == np.int32 and a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key
    assert [e['idf1'] for e in got['sequences']] == [e['idf1'] for e in want['sequences']] and got['all']['idf1'] == want['all']['idf1']


def both(labels, tracks, hota=False, **options):
    host = M.evaluate_sequences(labels, tracks, idf1=True, hota=hota, **options)
    device = M.evaluate_sequences(labels, tracks, device=True, idf1=True, hota=hota, **options)
    same_idf1(device, host)
    if hota:
        same_hota(device, host)
    return device


# ---------------------------------------------------------------------------------------------------- through evaluate_sequences
@pytest.mark.parametrize('hota', [False, True], ids=['alone', 'with_hota'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_named_cases_equal_the_host_form(name, hota):
    labels, tracks, _, options = CASES[name]
    e = both(labels, tracks, hota=hota, **options)['all']['idf1']
    if name == 'perfect':
        assert e == {'idf1': 1.0, 'idr': 1.0, 'idp': 1.0, 'integers': {'idtp': 10, 'idfn': 0, 'idfp': 0}}
    if name == 'swap':
        assert e['integers'] == {'idtp': 6, 'idfn': 4, 'idfp': 4}
    if name == 'threshold':
        assert e['integers'] == {'idtp': 1, 'idfn': 1, 'idfp': 1}
    if name == 'ignored':
        assert all(e[key] is None for key in I.RATIOS)


@pytest.mark.parametrize('hota', [False, True], ids=['alone', 'with_hota'])
@pytest.mark.parametrize('name', sorted(SCENES))
def test_hota_scenes_equal_the_host_form(name, hota):
    got = both(*SCENES[name](), hota=hota)
    if name == 'split':
        assert got['all']['idf1']['integers'] == {'idtp': 3, 'idfn': 3, 'idfp': 3} and got['all']['idf1']['idf1'] == 0.5
    if name == 'tie':
        assert got['idf1_pairs'][0]['C'].tolist() == [[4, 1]] and got['all']['idf1']['integers'] == {'idtp': 4, 'idfn': 0, 'idfp': 1}
    if name == 'dense_sequence':
        assert got['idf1_pairs'][0]['C'].shape == (128, 128) and got['idf1_pairs'][0]['C'].max() > 1


@pytest.mark.parametrize('hota', [False, True], ids=['alone', 'with_hota'])
def test_four_sequences_whole_and_in_chunks(monkeypatch, hota):
    """ in chunks of four frames the count rides every chunk of the one sweep and the assignment runs after the last: a count that missed
    a chunk, or an assignment that started early, would differ from the host form """
    scenes = [O.scene(41, frames=17, cars=9, quantum=16.0), (([], []), ([], [])), O.scene(42, frames=5, cars=20), O.dense(3, 30, 40)]
    labels, tracks = [s[0] for s in scenes], [s[1] for s in scenes]
    got = both(labels, tracks, hota=hota)
    assert got['seq_start'].tolist() == [0, 17, 17, 22, 23] and all(got['sequences'][1]['idf1'][key] is None for key in I.RATIOS)
    assert got['all']['idf1']['integers']['idtp'] == sum(e['idf1']['integers']['idtp'] for e in got['sequences']) > 0
    monkeypatch.setattr(kitti_eval, 'OVERLAP_WORKSPACE_BYTES', 4 * 40 * 32 * 8 * 4)        # four frames to a chunk: the same result
    assert kitti_eval.chunk_images(40, 32) == 4
    calls = []
    monkeypatch.setattr(hip, 'kitti_overlaps', lambda *a, _f=hip.kitti_overlaps: calls.append(1) or _f(*a))
    same_idf1(M.evaluate_sequences(labels, tracks, device=True, idf1=True, hota=hota), got)
    assert len(calls) == (12 if hota else 6)             # (23 frames in chunks of four: IDF1 alone never computes the overlaps again)


def test_every_metric():
    labels, tracks = O.scene(7, frames=4, cars=6)
    for metric in M.METRICS:
        got = both([labels], [tracks], metric=metric, min_overlap=0.25)
        assert got['all']['idf1']['integers']['idtp'] > 0 and got['params']['metric'] == metric


def test_tracker_tensors_are_scored_where_they_lie():
    labels, frames, removed = drive(5)
    rows, ids, _, _ = T.track_rows_device(torch.as_tensor(frames).cuda(), ('dist', 2.0))
    assert rows.is_cuda and ids.is_cuda
    got = M.evaluate_sequences([labels], [(rows, ids)], device=True, idf1=True)
    same_idf1(got, M.evaluate_sequences([labels], [(rows.cpu().numpy(), ids.cpu().numpy())], idf1=True))
    # the tracker keeps every identity: what is missing is what was removed
    assert got['all']['idf1']['integers'] == {'idtp': 6 * 30 - removed, 'idfn': removed, 'idfp': 0} and got['all']['idf1']['idp'] == 1.0


def test_without_idf1_the_device_result_is_todays():
    labels, tracks = O.scene(8, frames=3, cars=4)
    plain = M.evaluate_sequences([labels], [tracks], device=True)
    assert set(plain) == {'params', 'names', 'sequences', 'all', 'trajectories', 'frames', 'seq_start'} and 'idf1' not in plain['all']
    same_result(M.evaluate_sequences([labels], [tracks], device=True, idf1=False), plain)


def test_capped_workspace_is_a_value_error(monkeypatch):
    labels, tracks = O.scene(8, frames=3, cars=4)
    monkeypatch.setattr(PT, 'PAIR_TABLE_BYTES', 64)
    with pytest.raises(ValueError, match='device=False'):
        M.evaluate_sequences([labels], [tracks], device=True, idf1=True)
    monkeypatch.setattr(PT, 'PAIR_TABLE_BYTES', 1 << 30)
    monkeypatch.setattr(I, 'MAX_IDS', 3)
    with pytest.raises(ValueError, match='at most 3'):
        M.evaluate_sequences([labels], [tracks], device=True, idf1=True)


# ---------------------------------------------------------------------------------------------------- the assignment on written tables
def assign_written(tables, seed=0):
    """ the tables (with counters of any kind) written into a workspace, one gpp_idf1_assign -> per table (id_match, the seq_idf1 line) """
    rng = np.random.default_rng(seed)
    counters = [((C.sum(axis=1) + rng.integers(0, 3, C.shape[0])).astype(np.int32), (C.sum(axis=0) + rng.integers(0, 3, C.shape[1])).astype(np.int32))
                for C in tables]
    seq_tab, _, cells, vecs = PT.tables([0] * (len(tables) + 1), [C.shape[0] for C in tables], [C.shape[1] for C in tables])
    workspace = hip.idf1_workspace(cells, vecs, 0, len(tables), torch.device('cuda'))
    table, cnt = hip.idf1_tables(workspace, cells, vecs)
    for C, (gc, tc), (cell_base, n_gt, n_trk, vec_base, _, _) in zip(tables, counters, seq_tab.tolist()):
        table[cell_base:cell_base + n_gt * n_trk] = torch.as_tensor(np.ascontiguousarray(C).reshape(-1)).cuda()
        cnt[vec_base:vec_base + n_gt + n_trk] = torch.as_tensor(np.concatenate([gc, tc])).cuda()
    id_match, seq_idf1 = hip.idf1_assign(seq_tab.reshape(-1), cells, vecs, workspace)
    assert id_match.dtype == torch.int32 and tuple(id_match.shape) == (vecs,) and seq_idf1.dtype == torch.int64
    assert tuple(seq_idf1.shape) == (len(tables), hip.GPP_IDF1_SEQ_COLS)
    id_match, seq_idf1 = id_match.cpu().numpy(), seq_idf1.cpu().numpy()
    out = []
    for s, (cell_base, n_gt, n_trk, vec_base, _, _) in enumerate(seq_tab.tolist()):
        assert (id_match[vec_base + n_gt:vec_base + n_gt + n_trk] == -1).all()          # (the ids' entries are the caller's -1)
        out.append((id_match[vec_base:vec_base + n_gt], seq_idf1[s]))
    return out, counters


def check_written(tables, seed=0):
    got, counters = assign_written(tables, seed)
    for C, (gc, tc), (match, line) in zip(tables, counters, got):
        want_match, want_line = I.seq_counts_np(C, gc, tc)
        assert match.dtype == want_match.dtype and match.shape == want_match.shape and np.array_equal(match, want_match)
        assert line.dtype == want_line.dtype and line.tolist() == want_line.tolist()
        assert C.shape[0] * S - int(line[0]) == int(line[5]) == IO.rectangular_total(C)
    return got


SIDES = [(1, 1), (3, 5), (5, 3), (63, 64), (64, 65), (65, 64), (128, 300)]


@pytest.mark.parametrize('G,T', SIDES, ids=['{}x{}'.format(*s) for s in SIDES])
def test_written_tables_equal_the_host_form(G, T):
    """ padding columns and G > T; the lane's second column starts at 64; several columns a lane with a ragged last one -- sparse with
    competing rows, and dense with ties """
    check_written([IO.sparse_table(G * 131 + T, G, T, per_row=min(4, T), pool=max(1, min(G, T)))])
    check_written([IO.dense_table(G * 131 + T, G, T)])


def test_column_state_beyond_64_kib_of_lds():
    C = IO.sparse_table(7, 200, 3000, pool=220)          # 3008 columns of 24 bytes and 1024 rows of 8: 78 KiB
    got = check_written([C])
    assert (got[0][0] >= 0).sum() > 0 and (C > 0).sum(axis=1).max() <= 4


def test_both_limits():
    C = IO.cap_table()                                   # 1024 x 4096: 104 KiB of LDS
    got = check_written([C])
    assert got[0][1][6:].tolist() == [1024, 4096] and (C > 0).sum(axis=1).max() <= 4


def test_dense_256_with_ties():
    C = IO.dense_table(3, 256, 256)
    got = check_written([C])
    assert int(got[0][1][0]) == 2 * 256                  # (counts in {0, 1, 2}, a third of them 2: every trajectory finds a 2)


def test_an_all_zero_table():
    got = check_written([np.zeros((70, 90), np.int32)])
    assert got[0][1][0] == 0 and (got[0][0] == -1).all() and int(got[0][1][5]) == 70 * S


def test_sequences_of_different_sides_in_one_launch():
    """ LDS sized by the larger sequence, bases that are not zero, and sequences without trajectories or without ids between them """
    tables = [IO.sparse_table(1, 5, 3, per_row=2), np.zeros((0, 4), np.int32), IO.sparse_table(2, 128, 300, pool=140), np.zeros((3, 0), np.int32),
              IO.dense_table(4, 40, 7), IO.sparse_table(3, 7, 70, pool=9)]
    got = check_written(tables, seed=9)
    assert got[1][1].tolist()[:3] == [0, 0, got[1][1][4]] and got[3][0].tolist() == [-1] * 3 and got[3][1][0] == 0
    alone = [check_written([C], seed=9)[0] for C in tables]
    assert all(np.array_equal(a[0], b[0]) and a[1][0] == b[1][0] for a, b in zip(got, alone))


def test_count_then_assign_through_the_wrappers():
    """ the two launches as a caller of backend/hip.py would drive them: one frame, two labels, three rows """
    dev = torch.device('cuda')
    overlaps = torch.zeros((1, 4, 3, 2), dtype=torch.float64, device=dev)
    overlaps[0, 0] = torch.tensor([[0.5, 0.0], [0.75, 0.5], [float('nan'), np.nextafter(0.5, 0.0)]], dtype=torch.float64)
    lout, rout = torch.tensor([[1, 2]], dtype=torch.int32, device=dev), torch.tensor([[1, 3, 3]], dtype=torch.int32, device=dev)
    traj, trk = torch.tensor([[1, 0]], dtype=torch.int32, device=dev), torch.tensor([[2, 0, 1]], dtype=torch.int32, device=dev)
    seq_tab, frame_tab, cells, vecs = PT.tables([0, 1], [2], [3])
    workspace = hip.idf1_workspace(cells, vecs, 1, 1, dev)
    for _ in range(2):                                   # (the same frame twice: the counts add up)
        hip.idf1_count(overlaps, lout, rout, traj, trk, 0, frame_tab.reshape(-1), cells, vecs, workspace)
    table, cnt = hip.idf1_tables(workspace, cells, vecs)
    assert table.cpu().tolist() == [2, 0, 0, 2, 0, 2] and cnt.cpu().tolist() == [2, 2, 2, 2, 2]      # C[1] = (row 1, -, row 0); C[0] = (row 1, -, -)
    id_match, seq_idf1 = hip.idf1_assign(seq_tab.reshape(-1), cells, vecs, workspace)
    assert id_match.cpu().tolist() == [0, 2, -1, -1, -1] and seq_idf1.cpu().tolist() == [[4, 0, 2, 4, 6, 2 * S - 4, 2, 3]]


# ---------------------------------------------------------------------------------------------------- validation, nothing launched
def test_refusals_leave_the_outputs_alone():
    dev = torch.device('cuda')
    seq_tab, _, cells, vecs = PT.tables([0, 0], [2], [3])
    workspace = hip.idf1_workspace(cells, vecs, 0, 1, dev)
    id_match = torch.full((vecs,), 7, dtype=torch.int32, device=dev)
    seq_idf1 = torch.full((1, 8), 7, dtype=torch.int64, device=dev)
    lib, p = hip.lib(), hip.ptr
    tab = lambda lines: (ctypes.c_int32 * 6)(*lines)  # noqa: E731
    call = lambda lines, c=cells, v=vecs, w=workspace, n=None: lib.gpp_idf1_assign(  # noqa: E731
        tab(lines), 1, c, v, p(id_match), p(seq_idf1), p(w), int(w.numel()) if n is None else n, hip.stream_ptr())
    assert call([0, 2, 4, 0, 0, 0]) == -1 and call([1, 2, 3, 0, 0, 0]) == -1 and call([0, 2, 3, 1, 0, 0]) == -1 and call([0, -2, 3, 0, 0, 0]) == -1
    assert call([0, 1025, 1, 0, 0, 0], c=1025, v=1026) == -4 and call([0, 1, 4097, 0, 0, 0], c=4097, v=4098) == -4
    assert call([0, 2, 3, 0, 0, 0], n=64) == -2 and call([0, 2, 3, 0, 0, 0], w=workspace[4:]) == -3
    assert lib.gpp_idf1_assign(tab([0, 2, 3, 0, 0, 0]), 1, cells, vecs, None, p(seq_idf1), p(workspace), int(workspace.numel()), None) == -1
    assert lib.gpp_idf1_count(None, None, None, None, None, 1, 129, 4, 0, tab([0, 2, 3, 0, 0, 0]), cells, vecs, p(workspace), 256, None) == -4
    torch.cuda.synchronize()
    assert (id_match == 7).all() and (seq_idf1 == 7).all() and (workspace == 0).all()
    assert call([0, 2, 3, 0, 0, 0]) == 0                 # (and the same call, in order, runs)
    torch.cuda.synchronize()
    assert id_match.cpu().tolist() == [-1, -1, 7, 7, 7] and seq_idf1.cpu().tolist() == [[0, 0, 0, 0, 0, 2 * S, 2, 3]]
