""" The road-plane fit without a GPU (utils/road_fit.py): the NumPy form against the loop-written integer oracle
(tests/road_fit_oracle.py) on the clouds the GPU tests run, the mixer and the index draw pinned to hand-computed values, exact recovery of
a dyadic plane, independence of the chunking, and the files: scans, calibration, plane files, the command line.

Every comparison of the fit is for equality: it is integer arithmetic. """
import os

import numpy as np
import pytest

import road_fit_oracle as RO
from keras_retinanet_3D.bin import fit_plane_pool
from keras_retinanet_3D.utils import label_prep, road_fit

CASES = ['ragged', 'slab_h257', 'slab_h1', 'gates_h64', 'caps', 'exact', 'long_h3', 'slab_h1030']


def np_stages(name):
    """ every stage of the NumPy form on a case, in the oracle's layout """
    scans, Ts, ids, options = RO.cases()[name]
    o = road_fit.resolve_options(**options)
    q = [road_fit.quantise_np(p, T, o['region_q']) for p, T in zip(scans, Ts)]
    count = np.stack([road_fit.score_np(v, fid, o) for v, fid in zip(q, ids)])
    return q, count


@pytest.mark.parametrize('name', CASES)
def test_fit_np_equals_the_oracle(name):
    scans, Ts, ids, options = RO.cases()[name]
    o = road_fit.resolve_options(**options)
    want = RO.as_arrays(RO.expected(name), o['H'])
    q, count = np_stages(name)
    for f, v in enumerate(q):
        assert v.dtype == np.int32 and [tuple(r) for r in v.tolist()] == RO.expected(name)['q'][f]
    assert np.array_equal(count, want['count'])
    got = road_fit.fit_np(scans, Ts, ids, **options)
    for key in ('kept', 'winner', 'inliers', 'sums'):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert np.array_equal(got['valid'], ~np.isnan(got['planes']).any(axis=1)) and np.array_equal(got['valid'], ~np.isnan(got['rms']))
    assert not got['valid'][want['winner'] < 0].any()
    ok = got['planes'][got['valid']]
    assert np.allclose(np.linalg.norm(ok[:, :3], axis=1), 1.0, atol=1e-15) and (ok[:, 1] < 0).all()


def test_the_cases_hold_what_they_are_meant_to_hold():
    r = RO.as_arrays(RO.expected('ragged'), 300)
    assert [p.shape[0] for p in RO.cases()['ragged'][0]] == [0, 1, 255, 256, 257, 5000]
    assert r['kept'][0] == 0 and r['kept'][1] == 1 and r['kept'][2] == 0 and (r['kept'][3:] > 100).all()
    # the bounds: of every pair (on the bound, one quantum beyond) the first is kept; the NaN / infinite rows are not
    scans, Ts, _, options = RO.cases()['ragged']
    region = road_fit.resolve_options(**options)['region_q']
    assert region == (5120, 2048, 12800)
    kept = set(RO.expected('ragged')['q'][4])
    for p in ((5120, 256, 2560), (-5120, 256, 2560), (768, 2048, 2560), (768, -2048, 2560), (768, 256, 12800), (768, 256, 1)):
        assert p in kept
    assert not any(abs(x) > 5120 or abs(y) > 2048 or z < 1 or z > 12800 for x, y, z in kept)
    assert np.isnan(scans[4]).any() and np.isinf(scans[4]).any()
    s = RO.as_arrays(RO.expected('slab_h257'), 257)
    assert s['kept'].tolist() == [RO.SLAB - 1, RO.SLAB, RO.SLAB + 1, 0, 2, 3]
    assert (s['count'][3:5] == -1).all() and (s['count'][5] == -1).any() and (s['count'][5] == 3).any()      # repeated draws: n = 0
    g = RO.as_arrays(RO.expected('gates_h64'), 64)
    assert (g['count'][:3] == -1).all()                       # the wall and both heights: no valid hypothesis
    tie = g['count'][3]
    assert (tie[tie >= 0] == 600).all() and g['winner'][3] == int(np.argmax(tie >= 0)) and g['inliers'][3] == 600
    assert g['winner'][4] == -1 and g['inliers'][4] == 50 and not g['sums'][4].any()      # below min_inliers
    long = RO.as_arrays(RO.expected('long_h3'), 3)
    assert long['kept'][0] == 66 * RO.SLAB + 37 and (long['count'] >= 0).any() and long['winner'][0] >= 0
    c = RO.as_arrays(RO.expected('caps'), 300)
    q = np.array(RO.expected('caps')['q'][0])
    assert np.abs(q[:, 0]).max() == 10240 and np.abs(q[:, 1]).max() == 2048 and q[:, 2].max() == 20480 and (c['count'] >= 0).sum() > 200


def test_mixer_and_draw_are_pinned():
    # by hand: 1 -> (u ^= u >> 16) 1 -> (* 0x7feb352d) 0x7feb352d -> (u ^= u >> 15) 0x7febcafb -> (* 0x846ca68b) 0x6889f849 -> (u ^= u >> 16) 0x688990c0
    assert road_fit.mix(np.array([0, 1, 0xffffffff], np.uint32)).tolist() == [0, 0x688990c0, 0x6768824a]
    assert [RO.mix(v) for v in (0, 1, 0xffffffff)] == [0, 0x688990c0, 0x6768824a]
    # i_k = (mix(mix(mix(seed + frame) + h) + k) * m) >> 32
    assert road_fit.draw_indices(99, 0, 1, 5000).tolist() == [[759, 3031, 1969]]
    assert road_fit.draw_indices(0, 7481, 1024, 20000)[1023].tolist() == [13132, 18064, 19156]
    assert road_fit.draw_indices(4294967295, 4294967295, 6, 3)[5].tolist() == [0, 2, 2]      # seed + frame wraps around
    assert [RO.draw(0, 7481, 1023, k, 20000) for k in range(3)] == [13132, 18064, 19156]


def test_exact_recovery_of_a_dyadic_plane():
    case, truth, on_plane = RO.exact_case()
    scans, Ts, ids, options = case
    got = road_fit.fit_np(scans, Ts, ids, **options)
    count = RO.expected('exact')['count'][0]
    print('plane points {}, hypotheses with that count {}, winner {}, |plane - truth| {:.3g}'.format(
        on_plane, sum(1 for c in count if c == on_plane), got['winner'][0], np.abs(got['planes'][0] - truth).max()))
    assert got['kept'][0] == 5000 and max(count) == on_plane
    assert got['inliers'][0] == on_plane
    assert got['winner'][0] == next(h for h, c in enumerate(count) if c == on_plane)
    assert got['sums'][0][0] == on_plane
    # the centred moments are exact integers and each ratio is rounded once: the dyadic slopes and height come back exactly, the unit
    # normal to the round-off of one square root and a division
    assert np.abs(got['planes'][0] - truth).max() <= 1e-12
    assert got['rms'][0] == 0.0


def test_chunking_does_not_change_a_frame():
    scans, Ts, ids, options = RO.cases()['ragged']
    whole = road_fit.fit_np(scans, Ts, ids, **options)
    a = road_fit.fit_np(scans[:3], Ts[:3], ids[:3], **options)
    b = road_fit.fit_np(scans[3:], Ts[3:], ids[3:], **options)
    for key in whole:
        assert np.array_equal(whole[key], np.concatenate([a[key], b[key]]), equal_nan=True), key
    # the frame id, not the position, makes the draws
    moved = road_fit.fit_np(scans[5:], Ts[5:], [ids[5]], **options)
    other = road_fit.fit_np(scans[5:], Ts[5:], [ids[5] + 1], **options)
    assert np.array_equal(moved['sums'][0], whole['sums'][5]) and not np.array_equal(other['sums'][0], whole['sums'][5])


def test_solve_moments():
    # five points on y = 2 + x / 2 - z / 4 metres, in quanta
    pts = [(0, 512, 0), (256, 640, 0), (0, 448, 256), (512, 704, 256), (-256, 256, 512)]
    s = [sum(v) for v in zip(*[(1, x, y, z, x * x, x * z, z * z, x * y, z * y, y * y) for x, y, z in pts])]
    plane, rms = road_fit.solve_moments(s)
    norm = np.sqrt(0.25 + 1.0 + 0.0625)
    assert np.abs(plane - np.array([0.5, -1.0, -0.25, 2.0]) / norm).max() <= 1e-15 and rms == 0.0
    lifted = pts + [(0, 512 - 256, 0), (0, 512 + 256, 0)]      # one metre below and above one of them: the plane stays, the residual does not
    s2 = [sum(v) for v in zip(*[(1, x, y, z, x * x, x * z, z * z, x * y, z * y, y * y) for x, y, z in lifted])]
    plane2, rms2 = road_fit.solve_moments(s2)
    assert np.abs(plane2[:3] - plane[:3]).max() < 0.2 and 0.3 < rms2 < 0.7
    assert road_fit.solve_moments([2] + [0] * 9)[0] is None
    line = [(k, 300, 2 * k) for k in range(6)]                # collinear in (x, z): det = 0
    s3 = [sum(v) for v in zip(*[(1, x, y, z, x * x, x * z, z * z, x * y, z * y, y * y) for x, y, z in line])]
    assert road_fit.solve_moments(s3)[0] is None


def test_options_are_checked():
    o = road_fit.resolve_options()
    assert o['H'] == 1024 and o['region_q'] == (5120, 2048, 12800) and o['min_inliers'] == 100 and o['seed'] == 0
    assert o['tq2'] == 25.6 ** 2 and o['hlo2'] == 256.0 ** 2 and o['hhi2'] == 640.0 ** 2 and abs(o['c2'] - np.cos(np.radians(15.0)) ** 2) < 1e-15
    assert road_fit.resolve_options(region=(40, 8, 80))['region_q'] == (10240, 2048, 20480)
    for bad in (dict(region=(40.01, 8, 80)), dict(region=(20, 8.01, 50)), dict(region=(20, 8, 80.01)), dict(region=(20, 8, 0)), dict(region=(1, 2)),
                dict(region=(float('nan'), 8, 50)), dict(hypotheses=0), dict(min_inliers=0), dict(height=(2.0, 1.0)), dict(max_tilt=91),
                dict(threshold=-0.1), dict(seed=-1), dict(seed=1 << 32), dict(iterations=3)):
        with pytest.raises(ValueError):
            road_fit.resolve_options(**bad)
    with pytest.raises(ValueError):
        road_fit.fit_np([np.zeros((3, 4), np.float32)], [RO.PERMUTE], [0, 1])


# ---------------------------------------------------------------------------------------------------- files
def write_scans(root, scans, Ts):
    velo, calib = os.path.join(str(root), 'velodyne'), os.path.join(str(root), 'calib')
    os.makedirs(velo), os.makedirs(calib)
    for i, (p, T) in enumerate(zip(scans, Ts)):
        np.asarray(p, np.float32).tofile(os.path.join(velo, '%06d.bin' % i))
        with open(os.path.join(calib, '%06d.txt' % i), 'w') as f:
            f.write('P2: ' + ' '.join(['1.0'] * 12) + '\n')
            f.write('R0_rect: 1 0 0 0 1 0 0 0 1\n')
            f.write('Tr_velo_to_cam: ' + ' '.join(repr(float(v)) for v in np.asarray(T).ravel()) + '\n')
            f.write('Tr_imu_to_velo: ' + ' '.join(['0.5'] * 12) + '\n')
    return velo, calib


def test_scan_and_calibration_round_trip(tmp_path):
    scans, Ts, _, _ = RO.cases()['ragged']
    velo, calib = write_scans(tmp_path, scans, Ts)
    for i, (p, T) in enumerate(zip(scans, Ts)):
        got = road_fit.read_velodyne(os.path.join(velo, '%06d.bin' % i))
        assert got.dtype == np.float32 and got.shape == p.shape and np.array_equal(got, p, equal_nan=True)
        assert np.array_equal(road_fit.read_velo_calibration(os.path.join(calib, '%06d.txt' % i)), T)
    # R0_rect is applied: a rotation about z by 90 degrees swaps the first two rows
    path = os.path.join(str(tmp_path), 'rot.txt')
    with open(path, 'w') as f:
        f.write('R0_rect: 0 -1 0 1 0 0 0 0 1\nTr_velo_to_cam: 1 2 3 4 5 6 7 8 9 10 11 12\n')
    assert road_fit.read_velo_calibration(path).tolist() == [[-5, -6, -7, -8], [1, 2, 3, 4], [9, 10, 11, 12]]
    for text in ('R0_rect: 1 0 0 0 1 0 0 0 1\n', 'Tr_velo_to_cam: 1 2 3 4 5 6 7 8 9 10 11 12\n', 'R0_rect: 1 0 0\nTr_velo_to_cam: 1 2 3 4 5 6 7 8 9 10 11 12\n'):
        with open(path, 'w') as f:
            f.write(text)
        with pytest.raises(ValueError, match='rot.txt'):
            road_fit.read_velo_calibration(path)
    np.zeros(7, np.float32).tofile(path)
    with pytest.raises(ValueError, match='rot.txt'):
        road_fit.read_velodyne(path)


def test_read_plane_files(tmp_path):
    d = os.path.join(str(tmp_path), 'planes')
    os.makedirs(d)
    rows = [[-7.051729e-03, -9.997791e-01, -1.980151e-02, 1.680367e+00], [0.0, -1.0, 0.0, 1.65], [1.5e-02, -9.998e-01, 1.0e-03, 1.71]]
    for name, row in zip(('000002.txt', '000000.txt', '000001.txt'), rows):
        with open(os.path.join(d, name), 'w') as f:
            f.write('# Plane\nWidth 4\nHeight 1\n' + ' '.join('%.6e' % v for v in row) + '\n')
    pool, files = road_fit.read_plane_files(d)
    assert files == ['000000.txt', '000001.txt', '000002.txt'] and pool.dtype == np.float64
    assert np.array_equal(pool, np.array([rows[1], rows[2], rows[0]]))
    with open(os.path.join(d, '000003.txt'), 'w') as f:
        f.write('# Plane\nWidth 4\nHeight 1\n')
    with pytest.raises(ValueError, match='000003.txt'):
        road_fit.read_plane_files(d)


def test_fit_plane_pool_argument_errors(tmp_path, capsys):
    scans, Ts, _, _ = RO.cases()['gates_h64']
    velo, calib = write_scans(tmp_path, scans[3:], Ts[3:])
    out = os.path.join(str(tmp_path), 'pool.mat')
    empty = os.path.join(str(tmp_path), 'empty')
    os.makedirs(empty)
    for argv, text in (([os.path.join(str(tmp_path), 'nowhere'), calib, out, '--host'], 'no directory'),
                       ([empty, calib, out, '--host'], 'no .bin scans'),
                       ([velo, calib, out, '--host', '--region', '41', '8', '80'], 'region'),
                       ([velo, calib, out, '--host', '--hypotheses', '0'], 'hypotheses'),
                       ([velo, calib, out, '--host', '--height', '2', '1'], 'height'),
                       ([velo, empty, out, '--host'], '000000.txt'),
                       ([velo, calib, out, '--host', '--min-inliers', '601'], 'none of the 2 frames')):
        with pytest.raises(SystemExit) as e:
            fit_plane_pool.main(argv)
        assert isinstance(e.value.code, str) and e.value.code.startswith('fit_plane_pool: ') and text in e.value.code, e.value.code
        assert not os.path.exists(out)
    with pytest.raises(SystemExit) as e:                      # argparse's own: a usage message, exit status 2
        fit_plane_pool.main([velo, calib])
    assert e.value.code == 2
    capsys.readouterr()


def test_fit_plane_pool_on_the_host_writes_a_database(tmp_path, capsys):
    scans, Ts, ids, options = RO.cases()['gates_h64']
    velo, calib = write_scans(tmp_path, scans, Ts)
    out = os.path.join(str(tmp_path), 'pool.mat')
    result = fit_plane_pool.main([velo, calib, out, '--host', '--hypotheses', '64', '--seed', '2', '--report'])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 6 and sum('no plane' in line for line in lines) == 4 and '5 frames, 1 valid' in lines[-1]
    # frame_id is the position in the sorted list: the file's plane is that of fit_np with ids 0 .. 4
    want = road_fit.fit_np(scans, Ts, list(range(5)), hypotheses=64, seed=2)
    assert want['valid'].tolist() == [False, False, False, True, False]
    assert result['files'] == ['000003.bin'] and np.array_equal(result['planes'], want['planes'][3:4])
    for key in want:
        assert np.array_equal(result['record'][key], want[key], equal_nan=True), key
    truth = np.array([1.0 / 32, -1.0, 1.0 / 64, 1.5]) / np.sqrt(1.0 / 1024 + 1.0 + 1.0 / 4096)
    assert np.abs(result['planes'][0] - truth).max() <= 1e-12
    planes = label_prep._load_planes(out)
    assert planes.shape == (1, 4) and np.array_equal(planes, result['planes'].astype(np.float32))
    # chunks of two frames: the same pool
    again = road_fit.fit_pool(velo, calib, device=False, chunk_frames=2, hypotheses=64, seed=2)
    assert np.array_equal(again['planes'], result['planes']) and np.array_equal(again['record']['sums'], result['record']['sums'])


def test_device_entry_points_fail_loudly_without_a_gpu():
    import torch
    from keras_retinanet_3D.backend import hip
    if torch.cuda.is_available():
        return                                               # (tests/test_road_fit_gpu.py runs them)
    scans, Ts, ids, options = RO.cases()['gates_h64']
    with pytest.raises(hip.GppError):
        road_fit.fit_device(scans, Ts, ids, **options)
