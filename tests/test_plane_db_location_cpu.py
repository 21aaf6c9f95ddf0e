""" CPU: the host side of the distillation for the polled location error (utils/plane_db.py) -- select_polled_np against
the loop-written oracle of tests/plane_db_location_oracle.py, the properties of a run, signed gains, pair_costs_np against the key oracle
and against the host's pose recovery, the command line.  Every comparison is for equality. """
import os

import numpy as np
import pytest

import plane_db_location_oracle as QO
import plane_db_oracle as PO
from keras_retinanet_3D.bin import distil_planes
from keras_retinanet_3D.utils import gpp_utils, plane_db


def same(got, want):
    chosen, trace, best, cur, count = want
    assert got['chosen'].dtype == np.int32 and got['trace'].dtype == np.uint64 and got['best'].dtype == np.uint16 and got['cur'].dtype == np.uint16
    assert got['chosen'].tolist() == chosen and [int(v) for v in got['trace']] == trace
    assert got['best'].tolist() == best and got['cur'].tolist() == cur and got['count'] == count


def gains_at_every_pick(keys, errs, chosen):
    """ the (M,) int64 gain vectors that the picks of `chosen` saw, one per pick and one more for the state they leave """
    out = []
    for j in range(len(chosen) + 1):
        best, cur = plane_db.polled_state_np(keys, errs, chosen[:j])
        out.append(np.where(keys.astype(np.int64) < best.astype(np.int64)[:, None],
                            cur.astype(np.int64)[:, None] - errs.astype(np.int64), 0).sum(axis=0))
    return out


# ---------------------------------------------------------------------------------------------------- the selection
@pytest.mark.parametrize('M', [1, 7, 257])
@pytest.mark.parametrize('O', [1, 63, 64, 65, 300])
def test_select_polled_np_equals_the_loop_oracle(O, M):
    keys, errs = QO.seeded_pair(1000 * O + M, O, M)
    assert ((errs == 65535) == (keys == 65535)).all()
    if O * M >= 8:
        assert {0, 65534, 65535} <= set(errs.reshape(-1).tolist()) and {0, 57343, 65535} <= set(keys.reshape(-1).tolist())
    if O * M >= 63:
        assert 0.1 < (keys == 65535).mean() < 0.3
    k = min(M, 12 if O * M > 20000 else 40)
    got = plane_db.select_polled_np(keys, errs, k)
    same(got, QO.select_polled_loops(keys, errs, k))
    QO.check_result(keys, errs, k, got['chosen'], got['trace'], got['best'], got['cur'], got['count'])
    best, cur = plane_db.polled_state_np(keys, errs, got['chosen'])
    assert np.array_equal(best, got['best']) and np.array_equal(cur, got['cur'])
    assert best.tolist() == QO.replay_loops(keys, errs, got['chosen'][:got['count']])[0]


def test_of_duplicate_columns_the_first_wins_and_the_other_is_never_picked():
    keys, errs = QO.seeded_pair(5, 37, 7)
    keys[:, 1] = errs[:, 1] = 65535
    keys[:, 4], errs[:, 4] = np.minimum(keys[:, 4], 3000), np.minimum(errs[:, 4], 5)       # the clear winner ...
    keys[:, 2], errs[:, 2] = keys[:, 4], errs[:, 4]                                       # ... and its copy, at a lower index
    got = plane_db.select_polled_np(keys, errs, 7)
    same(got, QO.select_polled_loops(keys, errs, 7))
    assert got['chosen'][0] == 2 and 4 not in got['chosen'].tolist() and 1 not in got['chosen'].tolist()
    assert got['count'] < 7 and (got['chosen'][got['count']:] == -1).all()


def test_a_table_without_a_valid_pair_picks_nothing():
    keys = np.full((37, 7), 65535, np.uint16)
    got = plane_db.select_polled_np(keys, keys.copy(), 5)
    same(got, QO.select_polled_loops(keys, keys, 5))
    assert got['count'] == 0 and got['chosen'].tolist() == [-1] * 5 and got['trace'].tolist() == [65535 * 37] * 6
    assert (got['best'] == 65535).all() and (got['cur'] == 65535).all()
    assert plane_db.location_summary(got['cur'])['served'] == 0


def test_a_shorter_run_is_a_prefix_of_a_longer_one():
    keys, errs = QO.seeded_pair(9, 300, 257)
    ten, twenty = plane_db.select_polled_np(keys, errs, 10), plane_db.select_polled_np(keys, errs, 20)
    assert ten['count'] == 10 and twenty['count'] > 10
    assert np.array_equal(twenty['chosen'][:10], ten['chosen']) and np.array_equal(twenty['trace'][:11], ten['trace'])
    QO.check_result(keys, errs, 20, twenty['chosen'], twenty['trace'], twenty['best'], twenty['cur'], twenty['count'])


@pytest.mark.parametrize('O,M', [(63, 7), (300, 257), (1, 7)])
def test_the_first_pick_is_the_best_single_plane(O, M):
    keys, errs = QO.seeded_pair(31 + O + M, O, M)
    got = plane_db.select_polled_np(keys, errs, 1)
    single = [int(plane_db.polled_state_np(keys, errs, [p])[1].astype(np.int64).sum()) for p in range(M)]
    assert got['count'] == 1 and int(got['trace'][1]) == min(single) and got['chosen'][0] == single.index(min(single))


def test_some_pick_sees_a_negative_gain_and_the_picks_differ_from_the_key_greedy():
    """ the objective is not monotone: a plane that takes rows over with a smaller key and a larger error has a negative gain, and the
    picks part from the key greedy's """
    keys, errs = QO.seeded_pair(17, 65, 40)
    got = plane_db.select_polled_np(keys, errs, 40)
    gains = gains_at_every_pick(keys, errs, got['chosen'][:got['count']])
    assert any((g < 0).any() for g in gains[1:])                                          # (before the first pick every term is >= 0)
    for j in range(got['count']):
        assert got['chosen'][j] == int(np.argmax(gains[j])) and gains[j].max() > 0
        assert int(got['trace'][j]) - int(got['trace'][j + 1]) == gains[j].max()
    assert gains[got['count']].max() <= 0 or got['count'] == 40
    by_key = plane_db.select_np(keys, 40)
    assert got['chosen'].tolist() != by_key['chosen'].tolist()
    # under its own measure the polled rule's first pick is at least as good as the key greedy's
    assert int(got['trace'][1]) <= int(plane_db.polled_state_np(keys, errs, by_key['chosen'][:1])[1].astype(np.int64).sum())


def test_select_polled_np_and_the_replay_check_their_arguments():
    keys, errs = QO.seeded_pair(1, 4, 3)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            plane_db.select_polled_np(keys, errs, bad)
    with pytest.raises(ValueError):
        plane_db.select_polled_np(keys.astype(np.int32), errs, 1)
    with pytest.raises(ValueError):
        plane_db.select_polled_np(keys, errs[:, :2], 1)
    with pytest.raises(ValueError):
        plane_db.polled_state_np(keys, errs[:3], [0])


def test_location_summary_reads_metres_from_the_quanta():
    s = plane_db.location_summary(np.array([0, 256, 640, 65534, 65535], np.uint16))
    assert s == {'objects': 5, 'served': 4, 'mean_location_m': (0 + 256 + 640 + 65534) / 4 / 256.0, 'median_location_m': (256 + 640) / 2 / 256.0}


# ---------------------------------------------------------------------------------------------------- the cost tables
@pytest.fixture(scope='module')
def pairs():
    inp = QO.polling_inputs()
    keys, errs, loc, X = plane_db.pair_costs_np(inp['boxes'], inp['dims'], inp['orient'], inp['P_inv'], inp['want'], inp['pool'], return_locations=True)
    return dict(inp, keys=keys, errs=errs, loc=loc, X=X)


def test_pair_costs_np_keys_equal_the_key_oracle(pairs):
    keys, _, _, zc = PO.cost_keys(pairs['boxes'], pairs['dims'], pairs['orient'], pairs['P_inv'], pairs['pool'])
    assert pairs['keys'].dtype == np.uint16 and pairs['errs'].dtype == np.uint16 and pairs['keys'].shape == (10, QO.M_MAX)
    assert np.array_equal(pairs['keys'], keys)
    assert ((pairs['errs'] == 65535) == (keys == 65535)).all()
    pad, nan = QO.PAD_ROW[0] * 5 + QO.PAD_ROW[1], QO.NAN_ROW[0] * 5 + QO.NAN_ROW[1]
    assert (keys[pad] == 65535).all() and (keys[nan] == 65535).all()
    with np.errstate(invalid='ignore'):
        assert (zc[[r for r in range(10) if r not in (pad, nan)]] < 0).any()
    valid = pairs['errs'][keys != 65535]
    assert valid.max() == 65534 and valid.min() < 256 and (valid > 2560).any()            # centimetres to beyond the saturation
    # the quanta are the truncated distance, recomputed in float64 from the float32 locations (one quantum of slack for the rounding of
    # the float32 steps dist and dist * 256: an error of 1 ulp of a value below 65534 is below 0.004 quanta)
    dist = np.sqrt(((pairs['loc'].astype(np.float64) - pairs['want'].reshape(10, 1, 3).astype(np.float64)) ** 2).sum(axis=-1))
    ok = (keys != 65535) & np.isfinite(dist) & (dist * 256.0 < 65000.0)
    assert ok.sum() > 5000 and (np.abs(pairs['errs'][ok].astype(np.int64) - np.floor(dist[ok] * 256.0)) <= 1).all()


def test_the_location_is_the_one_of_the_hosts_pose_recovery(pairs):
    """ pair_costs_np's unquantised location against gpp_utils.recover_pose (the host path, pinned to the reference's goldens) on the
    same keypoints, over the rows within 100 m with finite values.  Measured here on the CPU over this test's 8045 seeded rows: the
    largest deviation is 0.0 -- np.cross forms the same three differences of products and np.linalg.norm's sum over three terms
    associates as (x x + y y) + z z, so the two paths round alike.  Four times the measured value is the bound: equality. """
    MEASURED = 0.0
    O, M = pairs['keys'].shape
    o = np.repeat(pairs['orient'].reshape(-1), M)
    with np.errstate(all='ignore'):
        det = gpp_utils.recover_pose({'keypoints': pairs['X'].reshape(-1, 4, 3), 'orientations': o, 'dimensions': np.repeat(pairs['dims'].reshape(-1, 3), M, axis=0)})
        ref = det['locations'].reshape(O, M, 3)
        loc = pairs['loc']
        ok = np.isfinite(ref).all(axis=-1) & np.isfinite(loc).all(axis=-1) & (np.abs(ref).max(axis=-1) < 100.0) & (o.reshape(O, M) >= 0)
        dev = np.abs(ref - loc).max(axis=-1)
    print('rows within 100 m: {}, largest deviation {!r} m'.format(int(ok.sum()), float(dev[ok].max())))
    assert ok.sum() > 5000 and ref.dtype == np.float32 and loc.dtype == np.float32
    assert dev[ok].max() <= 4 * MEASURED


# ---------------------------------------------------------------------------------------------------- command line and device
def test_command_line_reports_argument_errors(tmp_path, capsys):
    import scipy.io
    pool = os.path.join(str(tmp_path), 'pool.mat')
    scipy.io.savemat(pool, {'road_planes_database': np.tile(np.array([[0.0, -1.0, 0.0, 1.65]]), (5, 1))})
    out = os.path.join(str(tmp_path), 'out.mat')
    with pytest.raises(SystemExit):
        distil_planes.main([str(tmp_path), str(tmp_path), pool, out, '--planes', '2', '--objective', 'residual'])      # no such objective
    assert 'invalid choice' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        distil_planes.main([str(tmp_path), str(tmp_path), pool, out, '--planes', '6', '--objective', 'location'])
    assert '--planes 6 of a pool of 5' in str(e.value)
    assert not os.path.exists(out)
    assert distil_planes.parse_args(['a', 'b', 'c', 'd', '--planes', '3']).objective == 'poll'
    with pytest.raises(ValueError):
        plane_db.distil_rows([np.zeros((0, 16))], [np.eye(3, 4)], np.array([[0.0, -1.0, 0.0, 1.65]]), 1, objective='pose')


def test_objective_poll_prints_what_the_command_line_prints_today(tmp_path, capsys, monkeypatch):
    """ with --objective poll (and without the option) plane_db.distil is called as today -- no new argument -- and the lines are today's
    format, byte for byte """
    import scipy.io
    pool = os.path.join(str(tmp_path), 'pool.mat')
    planes = np.tile(np.array([[0.0, -1.0, 0.0, 1.65]]), (12, 1)) + np.arange(12)[:, None] * 0.01
    scipy.io.savemat(pool, {'road_planes_database': planes})
    calls = []

    def fake_distil(label_dir, calib_dir, pool_arg, k, **kw):
        calls.append(kw)
        trace = np.array([65535 * 7] + [1000 - 10 * j for j in range(k)], np.uint64)
        out = {'planes': planes[:k], 'indices': np.arange(k, dtype=np.int32), 'trace': trace, 'count': k, 'objects': 7,
               'best': np.zeros(7, np.uint16), 'served': 7, 'six_vote_share': 0.5, 'median_residual_m': 0.0123}
        if kw.get('objective') == 'location':
            out.update(objective='location', cur=np.full(7, 128, np.uint16), mean_location_m=0.5, median_location_m=0.5)
        return out
    monkeypatch.setattr(plane_db, 'distil', fake_distil)
    outs = []
    for extra in ([], ['--objective', 'poll'], ['--objective', 'location']):
        out = os.path.join(str(tmp_path), 'out{}.mat'.format(len(outs)))
        distil_planes.main(['l', 'c', pool, out, '--planes', '11'] + extra)
        outs.append(capsys.readouterr().out.replace(out, 'OUT'))
    assert calls[0] == calls[1] == {'det_types': 1, 'report': False} and calls[2] == {'det_types': 1, 'report': False, 'objective': 'location'}
    today = ('{:8d} planes   objective {:16d}   per object {:10.2f}\n'.format(1, 1000, 1000 / 7)
             + '{:8d} planes   objective {:16d}   per object {:10.2f}\n'.format(10, 910, 910 / 7)
             + '{:8d} planes   objective {:16d}   per object {:10.2f}   six votes {:7.2%}   median residual {:.4f} m\n'.format(11, 900, 900 / 7, 0.5, 0.0123)
             + 'OUT: 11 of 12 planes, 7 objects\n')
    assert outs[0] == today and outs[1] == today
    lines = outs[2].splitlines()
    assert len(lines) == 4 and 'per object {:10.4f} m'.format(900 / 256.0 / 7) in lines[2] and 'location error mean 0.500 m   median 0.500 m' in lines[2]
    assert 'six votes' not in outs[2]


def test_device_entry_points_fail_loudly_without_a_gpu():
    import torch
    from keras_retinanet_3D.backend import hip
    if torch.cuda.is_available():
        return                                               # (tests/test_plane_db_location_gpu.py runs them)
    P = np.array([[700.0, 0, 600, 0], [0, 700.0, 180, 0], [0, 0, 1, 0]])
    with pytest.raises(hip.GppError):
        plane_db.distil_rows([np.zeros((0, 16))], [P], np.array([[0.0, -1.0, 0.0, 1.65]]), 1, objective='location')
    with pytest.raises(hip.GppError):
        plane_db.cost_table([np.zeros((0, 16))], [P], np.array([[0.0, -1.0, 0.0, 1.65]]), errors=True)
