""" Several road planes per frame without a GPU (utils/road_fit.py): the NumPy form against the loop-written oracle
(tests/road_fit_rounds_oracle.py) at every stage of every round, round 0 against fit_np, the round seed pinned by hand, independence of
chunking and position, the two-level recovery, the share gate, and the command line.

Every comparison of the fit is for equality: it is integer arithmetic. """
import os

import numpy as np
import pytest

import road_fit_oracle as RO
import road_fit_rounds_oracle as RR
from keras_retinanet_3D.bin import fit_plane_pool
from keras_retinanet_3D.utils import label_prep, road_fit

CASES = ['two_level', 'share_gate', 'ragged', 'gates_h64', 'slab_h257']
KEYS = ('kept', 'count', 'winner', 'inliers', 'sums')


def case(name):
    if name == 'two_level':
        return RR.two_level_frames()
    if name == 'share_gate':
        return RR.share_gate_frame()
    return RO.cases()[name]


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype == np.float64:
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))
    else:
        assert np.array_equal(a, b)


@pytest.mark.parametrize('name', CASES)
def test_fit_rounds_np_equals_the_oracle_at_every_stage_of_every_round(name):
    scans, Ts, ids, options = case(name)
    o = road_fit.resolve_options(**options)
    want = RR.expected_rounds(name)
    got = road_fit.np_round_stages(scans, Ts, ids, 3, **options)
    assert len(got) == len(want) == 3
    for r in range(3):
        w = RR.as_arrays(want[r], o['H'])
        for f, v in enumerate(got[r]['q']):
            assert v.dtype == np.int32 and [tuple(p) for p in v.tolist()] == want[r]['q'][f], (r, f)
        for key in KEYS:
            assert got[r][key].dtype == w[key].dtype and np.array_equal(got[r][key], w[key]), (r, key)
    # the peel's invariant: what a round takes out is what its moments counted
    for r in range(2):
        has = got[r]['winner'] >= 0
        assert np.array_equal((got[r]['kept'] - got[r + 1]['kept'])[has], got[r]['sums'][has, 0])
        assert not got[r + 1]['kept'][~has].any()
    # the host's step against the oracle's, for the default share and for none
    for share in (0.10, 0.0):
        fit = road_fit.fit_rounds_np(scans, Ts, ids, 3, share, **options)
        for f in range(len(scans)):
            flags = RR.validity(want[0]['kept'][f], [want[r]['winner'][f] for r in range(3)], [want[r]['inliers'][f] for r in range(3)],
                                [want[r]['sums'][f] for r in range(3)], share)
            assert fit['valid'][f].tolist() == flags, (share, f)
        assert np.array_equal(fit['valid'], ~np.isnan(fit['planes']).any(axis=2)) and np.array_equal(fit['valid'], ~np.isnan(fit['rms']))
        for key in ('kept', 'winner', 'inliers', 'sums'):
            assert np.array_equal(fit[key], np.stack([got[r][key] for r in range(3)], axis=1)), key


@pytest.mark.parametrize('P', [1, 3])
def test_round_0_is_fit_np(P):
    scans, Ts, ids, options = RO.cases()['ragged']
    one = road_fit.fit_np(scans, Ts, ids, **options)
    got = road_fit.fit_rounds_np(scans, Ts, ids, P, **options)
    assert sorted(got) == sorted(one)
    for key in one:
        assert got[key].shape[:2] == (len(scans), P), key
        same_bits(np.ascontiguousarray(got[key][:, 0]), one[key])


def test_round_seed_is_pinned():
    assert road_fit.ROUND_SEED_STEP == 0x9e3779b9
    assert road_fit.round_seed(0, 0) == 0 and road_fit.round_seed(5, 0) == 5 and road_fit.round_seed(0, 1) == 0x9e3779b9
    assert road_fit.round_seed(0xffffffff, 1) == 0x9e3779b8          # 0xffffffff + 0x9e3779b9 = 0x1_9e3779b8
    assert road_fit.round_seed(1, 2) == 0x3c6ef373                  # 1 + 2 * 0x9e3779b9 = 0x1_3c6ef373
    assert road_fit.round_seed(7, 3) == (7 + 3 * 0x9e3779b9) - (1 << 32) == 0xdaa66d32
    assert [RR.round_seed(s, r) for s, r in ((0xffffffff, 1), (1, 2), (7, 3))] == [0x9e3779b8, 0x3c6ef373, 0xdaa66d32]


def test_chunking_and_position_do_not_change_a_frame():
    scans, Ts, ids, options = RO.cases()['ragged']
    whole = road_fit.fit_rounds_np(scans, Ts, ids, 3, **options)
    assert whole['valid'][:, 0].sum() >= 2 and (whole['winner'][:, 1] >= 0).any()
    a = road_fit.fit_rounds_np(scans[:3], Ts[:3], ids[:3], 3, **options)
    b = road_fit.fit_rounds_np(scans[3:], Ts[3:], ids[3:], 3, **options)
    for key in whole:
        assert np.array_equal(whole[key], np.concatenate([a[key], b[key]]), equal_nan=True), key
    moved = road_fit.fit_rounds_np(scans[::-1], Ts[::-1], ids[::-1], 3, **options)
    for key in whole:
        assert np.array_equal(whole[key], moved[key][::-1], equal_nan=True), key
    other = road_fit.fit_rounds_np(scans[5:], Ts[5:], [ids[5] + 1], 3, **options)      # the frame id, not the position, makes the draws
    assert not np.array_equal(other['sums'][0], whole['sums'][5])


def test_two_levels_are_recovered_exactly():
    scans, Ts, ids, options = RR.two_level_frames()
    assert len(scans) == 20 and ids == list(range(20)) and options == dict(hypotheses=64)
    got = road_fit.fit_rounds_np(scans, Ts, ids, 3, **options)
    truth = RR.two_level_truth().reshape(20, 2, 4)
    assert (got['kept'] == [650, 250, 0]).all() and (got['inliers'] == [400, 250, 0]).all()
    assert (got['winner'][:, :2] >= 0).all() and (got['winner'][:, 2] == -1).all()
    assert (got['valid'] == [True, True, False]).all()
    assert np.array_equal(got['planes'][:, 0], truth[:, 0]) and np.array_equal(got['planes'][:, 1], truth[:, 1])
    assert (got['rms'][:, :2] == 0.0).all()
    assert np.array_equal(got['planes'][got['valid']], RR.two_level_truth())            # the pool: (frame, round) order


def test_the_share_gate():
    scans, Ts, ids, options = RR.share_gate_frame()
    assert options['min_inliers'] == 30
    gated = road_fit.fit_rounds_np(scans, Ts, ids, 3, **options)                         # min_share = 0.10: ceil(0.1 * 690) = 70 (0.1 > 1/10)
    assert gated['kept'].tolist() == [[690, 290, 40]] and gated['inliers'].tolist() == [[400, 250, 40]]
    assert gated['winner'][0, 2] >= 0 and gated['valid'].tolist() == [[True, True, False]] and np.isnan(gated['planes'][0, 2]).all()
    free = road_fit.fit_rounds_np(scans, Ts, ids, 3, 0.0, **options)
    assert free['valid'].tolist() == [[True, True, True]] and np.array_equal(free['planes'][0, 2], [0.0, -1.0, 0.0, 1.625])
    for key in ('kept', 'winner', 'inliers', 'sums'):
        assert np.array_equal(free[key], gated[key]), key
    # validity is a prefix: a round-1 count below the share takes round 2 with it, whatever round 2 counted
    s = free['sums'].copy()
    for inliers, share, want in (([400, 50, 300], 0.10, [True, False, False]), ([400, 69, 300], 0.10, [True, False, False]),
                                 ([400, 70, 70], 0.10, [True, True, True]), ([400, 300, 50], 0.10, [True, True, False]),
                                 ([10, 300, 300], 0.10, [True, True, True]), ([400, 690, 690], 1.0, [True, True, True]),
                                 ([400, 689, 690], 1.0, [True, False, False])):
        got = road_fit._assemble_rounds(free['kept'], free['winner'], np.array([inliers], np.int32), s, share)
        assert got['valid'].tolist() == [want], (inliers, share)
        assert RR.validity(690, free['winner'][0].tolist(), inliers, s[0], share) == want
    no_winner = road_fit._assemble_rounds(free['kept'], np.array([[4, -1, 0]], np.int32), free['inliers'], s, 0.0)
    assert no_winner['valid'].tolist() == [[True, False, False]]
    for bad in (dict(planes_per_frame=0), dict(planes_per_frame=17), dict(planes_per_frame=1.5), dict(planes_per_frame=2, min_share=1.5),
                dict(planes_per_frame=2, min_share=-0.1), dict(planes_per_frame=2, min_share=float('nan'))):
        with pytest.raises(ValueError):
            road_fit.fit_rounds_np(scans, Ts, ids, **dict(bad, **options))
    with pytest.raises(ValueError):                           # the options stay DEFAULTS': the new names are parameters, not options
        road_fit.resolve_options(planes_per_frame=2)


def test_chunks_count_the_second_point_buffer():
    sizes = [1000] * 10
    assert road_fit._chunks(sizes, 64, 64, 28 * 1000 * 5 + 5 * (4 * 64 + 256)) == [(0, 5), (5, 10)]
    assert road_fit._chunks(sizes, 64, 64, 28 * 1000 * 5 + 5 * (4 * 64 + 256), 40) == [(0, 3), (3, 6), (6, 9), (9, 10)]


# ---------------------------------------------------------------------------------------------------- files
def write_scans(root, scans, Ts):
    velo, calib = os.path.join(str(root), 'velodyne'), os.path.join(str(root), 'calib')
    os.makedirs(velo), os.makedirs(calib)
    for i, (p, T) in enumerate(zip(scans, Ts)):
        np.asarray(p, np.float32).tofile(os.path.join(velo, '%06d.bin' % i))
        with open(os.path.join(calib, '%06d.txt' % i), 'w') as f:
            f.write('R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: ' + ' '.join(repr(float(v)) for v in np.asarray(T).ravel()) + '\n')
    return velo, calib


def test_fit_pool_with_one_plane_per_frame_is_todays(tmp_path):
    scans, Ts, ids, options = RR.two_level_frames()
    velo, calib = write_scans(tmp_path, scans[:4], Ts[:4])
    a = road_fit.fit_pool(velo, calib, device=False, hypotheses=64)
    b = road_fit.fit_pool(velo, calib, device=False, hypotheses=64, planes_per_frame=1, min_share=0.5)
    assert sorted(a) == sorted(b) == ['files', 'frames', 'planes', 'record'] and a['record']['planes'].shape == (4, 4)
    assert a['planes'].tobytes() == b['planes'].tobytes() and a['files'] == b['files']
    assert np.array_equal(a['planes'], RR.two_level_truth()[0:8:2])


def test_the_command_line_with_two_planes_per_frame(tmp_path, capsys):
    scans, Ts, ids, options = RR.two_level_frames()
    velo, calib = write_scans(tmp_path, scans[:4], Ts[:4])
    out = os.path.join(str(tmp_path), 'pool.mat')
    result = fit_plane_pool.main([velo, calib, out, '--host', '--hypotheses', '64', '--planes-per-frame', '2', '--report'])
    lines = capsys.readouterr().out.splitlines()
    truth = RR.two_level_truth()[:8]
    assert np.array_equal(result['planes'], truth) and result['rounds'].dtype == np.int32 and result['rounds'].tolist() == [0, 1] * 4
    assert result['files'] == [n for i in range(4) for n in ['%06d.bin' % i] * 2] and result['frames'] == ['%06d.bin' % i for i in range(4)]
    assert result['record']['planes'].shape == (4, 2, 4)
    assert np.array_equal(label_prep._load_planes(out), truth.astype(np.float32))
    assert len(lines) == 9 and lines[-1].startswith(out + ': 4 frames, 4 valid, 8 planes, median inliers ')
    for i, line in enumerate(lines[:8]):
        f, r = divmod(i, 2)
        assert line.startswith('%06d.bin  round %d  kept %7d  inliers %7d  rms 0.0000 m  plane ' % (f, r, (650, 250)[r], (400, 250)[r])), line
        assert line.endswith('%+.6f %+.6f %+.6f %+.6f' % tuple(truth[i])), line
    # a third round finds nothing: 'no plane' lines, the same pool; chunks of one frame: the same pool
    again = fit_plane_pool.main([velo, calib, out, '--host', '--hypotheses', '64', '--planes-per-frame', '3', '--report'])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 13 and sum('no plane' in line for line in lines) == 4 and '4 frames, 4 valid, 8 planes' in lines[-1]
    assert np.array_equal(again['planes'], truth)
    chunked = road_fit.fit_pool(velo, calib, device=False, chunk_frames=1, planes_per_frame=2, hypotheses=64)
    assert np.array_equal(chunked['planes'], truth) and chunked['files'] == result['files']
    # one plane per frame: the lines of before, no 'planes' in the summary
    fit_plane_pool.main([velo, calib, out, '--host', '--hypotheses', '64', '--report'])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 5 and 'round' not in lines[0] and lines[-1].startswith(out + ': 4 frames, 4 valid, median inliers 400')


def test_the_command_line_refuses_bad_values(tmp_path, capsys):
    scans, Ts, ids, options = RR.two_level_frames()
    velo, calib = write_scans(tmp_path, scans[:1], Ts[:1])
    out = os.path.join(str(tmp_path), 'pool.mat')
    for argv, text in ((['--planes-per-frame', '0'], 'planes_per_frame'), (['--planes-per-frame', '17'], 'planes_per_frame'),
                       (['--min-share', '1.5'], 'min_share'), (['--planes-per-frame', '2', '--min-share', '-0.5'], 'min_share')):
        with pytest.raises(SystemExit) as e:
            fit_plane_pool.main([velo, calib, out, '--host'] + argv)
        assert isinstance(e.value.code, str) and e.value.code.startswith('fit_plane_pool: ') and text in e.value.code, e.value.code
        assert not os.path.exists(out)
    capsys.readouterr()


def test_the_device_form_fails_loudly_without_a_gpu():
    import torch
    from keras_retinanet_3D.backend import hip
    if torch.cuda.is_available():
        return                                               # (tests/test_road_fit_rounds_gpu.py runs it)
    scans, Ts, ids, options = RR.share_gate_frame()
    with pytest.raises(hip.GppError):
        road_fit.fit_rounds_device(scans, Ts, ids, 2, **options)
