""" CPU: the host side of the plane distillation (utils/plane_db.py) -- select_np against the loop-written oracle of
tests/plane_db_oracle.py, the properties of a run, the .mat round trip and the command line's argument errors. """
import os

import numpy as np
import pytest

import plane_db_oracle as PO
from keras_retinanet_3D.bin import distil_planes
from keras_retinanet_3D.utils import label_prep, plane_db


def same(got, want):
    chosen, trace, best, count = want
    assert got['chosen'].dtype == np.int32 and got['trace'].dtype == np.uint64 and got['best'].dtype == np.uint16
    assert got['chosen'].tolist() == chosen and [int(v) for v in got['trace']] == trace and got['best'].tolist() == best and got['count'] == count


@pytest.mark.parametrize('M', [1, 7, 300])
@pytest.mark.parametrize('O', [1, 37, 1000])
def test_select_np_equals_the_loop_oracle(O, M):
    table = PO.seeded_table(1000 * O + M, O, M)
    if O * M > 1:
        assert {0, 57343, 65535} <= set(table.reshape(-1).tolist())
    k = min(M, 12 if O == 1000 else 40)
    got = plane_db.select_np(table, k)
    same(got, PO.select_loops(table, k))
    PO.check_result(table, k, got['chosen'], got['trace'], got['best'], got['count'])


def test_of_duplicate_columns_the_first_wins_and_the_other_is_never_picked():
    table = PO.seeded_table(5, 37, 7)
    table[:, 1] = 65535
    table[:, 4] = np.minimum(table[:, 4], 3000)              # the clear winner ...
    table[:, 2] = table[:, 4]                                # ... and its copy, at a lower index
    got = plane_db.select_np(table, 7)
    same(got, PO.select_loops(table, 7))
    assert got['chosen'][0] == 2 and 4 not in got['chosen'].tolist() and 1 not in got['chosen'].tolist()
    assert got['count'] < 7 and (got['chosen'][got['count']:] == -1).all()


def test_a_table_without_a_valid_pair_picks_nothing():
    table = np.full((37, 7), 65535, np.uint16)
    got = plane_db.select_np(table, 5)
    same(got, PO.select_loops(table, 5))
    assert got['count'] == 0 and got['chosen'].tolist() == [-1] * 5 and got['trace'].tolist() == [65535 * 37] * 6
    assert (got['best'] == 65535).all()


@pytest.mark.parametrize('O,M', [(37, 7), (1, 300), (37, 300)])
def test_a_run_to_exhaustion_ends_at_the_column_minimum_sum(O, M):
    table = PO.seeded_table(77 + O + M, O, M)
    got = plane_db.select_np(table, M)
    if O * M <= 37 * 7 or O == 1:
        same(got, PO.select_loops(table, M))
    PO.check_result(table, M, got['chosen'], got['trace'], got['best'], got['count'])
    assert int(got['trace'][-1]) == int(table.min(axis=1).astype(np.int64).sum())
    assert plane_db.objective(table, got['chosen']) == int(got['trace'][-1])


def test_a_shorter_run_is_a_prefix_of_a_longer_one():
    table = PO.seeded_table(9, 1000, 300)
    ten, twenty = plane_db.select_np(table, 10), plane_db.select_np(table, 20)
    assert ten['count'] == 10 and twenty['count'] == 20
    assert np.array_equal(twenty['chosen'][:10], ten['chosen']) and np.array_equal(twenty['trace'][:11], ten['trace'])
    PO.check_result(table, 20, twenty['chosen'], twenty['trace'], twenty['best'], twenty['count'])


def test_select_np_checks_its_arguments():
    table = PO.seeded_table(1, 4, 3)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            plane_db.select_np(table, bad)
    with pytest.raises(ValueError):
        plane_db.select_np(table.astype(np.int32), 1)


def test_best_summary_reads_votes_and_residual_from_the_keys():
    best = np.array([0, 614, 8191, 8192 + 1024, 65535], np.uint16)        # three six-vote objects, one five-vote, one unserved
    s = plane_db.best_summary(best)
    assert s['objects'] == 5 and s['served'] == 4 and s['six_vote_share'] == 3 / 5
    assert s['median_residual_m'] == np.median([0.0, 614 / 1024 / 6, 8191 / 1024 / 6, 1.0 / 6])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_a_written_database_reads_back(tmp_path, dtype):
    planes = np.random.default_rng(3).normal(size=(13, 4)).astype(dtype)
    path = os.path.join(str(tmp_path), 'db.mat')
    plane_db.write_database(path, planes)
    import scipy.io
    raw = scipy.io.loadmat(path)['road_planes_database']
    assert raw.dtype == dtype and np.array_equal(raw, planes)
    assert np.array_equal(label_prep._load_planes(path), planes.astype(np.float32))
    with pytest.raises(ValueError):
        plane_db.write_database(path, np.zeros((0, 4)))


def test_command_line_reports_argument_errors(tmp_path, capsys):
    import scipy.io
    pool, empty = os.path.join(str(tmp_path), 'pool.mat'), os.path.join(str(tmp_path), 'empty.mat')
    scipy.io.savemat(pool, {'road_planes_database': np.tile(np.array([[0.0, -1.0, 0.0, 1.65]]), (5, 1))})
    scipy.io.savemat(empty, {'road_planes_database': np.zeros((0, 4))})
    out = os.path.join(str(tmp_path), 'out.mat')
    with pytest.raises(SystemExit) as e:
        distil_planes.main([str(tmp_path), str(tmp_path), pool, out, '--planes', '6'])
    assert '--planes 6 of a pool of 5' in str(e.value)
    with pytest.raises(SystemExit) as e:
        distil_planes.main([str(tmp_path), str(tmp_path), empty, out, '--planes', '1'])
    assert 'holds no (M, 4) pool' in str(e.value)
    with pytest.raises(SystemExit):
        distil_planes.main([str(tmp_path), str(tmp_path), pool, out])                      # --planes is required
    assert not os.path.exists(out)


def test_device_entry_points_fail_loudly_without_a_gpu():
    import torch
    from keras_retinanet_3D.backend import hip
    if torch.cuda.is_available():
        return                                               # (tests/test_plane_db_gpu.py runs them)
    P = np.array([[700.0, 0, 600, 0], [0, 700.0, 180, 0], [0, 0, 1, 0]])
    with pytest.raises(hip.GppError):
        plane_db.distil_rows([np.zeros((0, 16))], [P], np.array([[0.0, -1.0, 0.0, 1.65]]), 1)
