""" The road-plane fit on the GPU (csrc/road_fit.hip): every launch against the NumPy form (utils/road_fit.py) and the
loop-written integer oracle (tests/road_fit_oracle.py), the whole fit in one chunk and in several, a second run in the same process, and
the chain scan -> pool -> database -> polling.

Every comparison is for equality: the fit is integer arithmetic and documented single float64 operations. """
import ctypes
import os

import numpy as np
import pytest
import torch

import label_prep_oracle as LO
import road_fit_oracle as RO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.bin import fit_plane_pool
from keras_retinanet_3D.utils import plane_db, road_fit
from keras_retinanet_3D.utils import label_prep as L

pytestmark = pytest.mark.gpu

CASES = ['ragged', 'slab_h257', 'slab_h1', 'gates_h64', 'caps', 'exact', 'long_h3', 'slab_h1030']


@pytest.fixture(scope='module')
def stages():
    """ the four launches on every case, fetched once """
    return {name: road_fit.device_stages(*RO.cases()[name][:3], **RO.cases()[name][3]) for name in CASES}


def want_of(name):
    scans, Ts, ids, options = RO.cases()[name]
    o = road_fit.resolve_options(**options)
    return o, RO.as_arrays(RO.expected(name), o['H']), RO.expected(name)['q']


@pytest.mark.parametrize('name', CASES)
def test_points_equal_the_oracle_and_numpy(stages, name):
    scans, Ts, ids, options = RO.cases()[name]
    o, want, want_q = want_of(name)
    got = stages[name]
    assert got['kept'].dtype == np.int32 and np.array_equal(got['kept'], want['kept'])
    for f, (p, T) in enumerate(zip(scans, Ts)):
        a, m = int(got['offsets'][f]), int(want['kept'][f])
        mine = got['q'][a:a + m]
        assert [tuple(r) for r in mine.tolist()] == want_q[f]            # the kept points, in the scan's order
        assert np.array_equal(mine, road_fit.quantise_np(p, T, o['region_q']))
        assert not got['q'][a + m:int(got['offsets'][f + 1])].any()      # the rest of the frame's segment is not written


@pytest.mark.parametrize('name', CASES)
def test_score_equals_the_oracle_and_numpy(stages, name):
    scans, Ts, ids, options = RO.cases()[name]
    o, want, _ = want_of(name)
    got = stages[name]['count']
    assert got.dtype == np.int32 and got.shape == want['count'].shape and np.array_equal(got, want['count'])
    for f, (p, T, fid) in enumerate(zip(scans, Ts, ids)):
        assert np.array_equal(got[f], road_fit.score_np(road_fit.quantise_np(p, T, o['region_q']), fid, o))


@pytest.mark.parametrize('H', [64, 300, 600, 1024, 1025])
def test_score_of_other_hypothesis_counts_is_a_prefix(stages, H):
    """ H = 1, 257 and 1030 are cases of their own (less than a wavefront, one lane into a second workgroup, a fifth workgroup); 64, 300,
    600, 1024 and 1025 on the slab frames against the NumPy form: hypothesis h does not depend on H """
    scans, Ts, ids, options = RO.cases()['slab_h257']
    got = road_fit.device_stages(scans, Ts, ids, **dict(options, hypotheses=H))['count']
    o = road_fit.resolve_options(**dict(options, hypotheses=H))
    want = np.stack([road_fit.score_np(road_fit.quantise_np(p, T, o['region_q']), fid, o) for p, T, fid in zip(scans, Ts, ids)])
    assert np.array_equal(got, want)
    n = min(H, 1030)
    assert np.array_equal(got[:, :n], stages['slab_h1030']['count'][:, :n])


@pytest.mark.parametrize('name', CASES)
def test_winner_and_moments_equal_the_oracle_and_numpy(stages, name):
    scans, Ts, ids, options = RO.cases()[name]
    o, want, _ = want_of(name)
    got = stages[name]
    for key in ('winner', 'inliers', 'sums'):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    for f, (p, T, fid) in enumerate(zip(scans, Ts, ids)):
        q = road_fit.quantise_np(p, T, o['region_q'])
        w, c = road_fit.winner_np(got['count'][f], o['min_inliers'])
        assert (w, c) == (got['winner'][f], got['inliers'][f])
        assert np.array_equal(road_fit.moments_np(q, fid, w, o), got['sums'][f])
        if w < 0:
            assert not got['sums'][f].any()


def test_ties_take_the_first_hypothesis_and_a_thin_frame_has_no_plane(stages):
    g = stages['gates_h64']
    tie = g['count'][3]
    assert (tie[tie >= 0] == 600).all() and (tie >= 0).sum() > 1 and g['winner'][3] == int(np.argmax(tie >= 0)) and g['sums'][3][0] == 600
    assert (g['count'][:3] == -1).all() and (g['winner'][:3] == -1).all() and (g['inliers'][:3] == 0).all()
    assert g['winner'][4] == -1 and g['inliers'][4] == 50 and not g['sums'][4].any()


def same_fit(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        if a[key].dtype == np.float64:                        # bit for bit; the NaN rows are the canonical NaN on both sides
            assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])), key
            assert np.array_equal(a[key][~np.isnan(a[key])].view(np.uint64), b[key][~np.isnan(b[key])].view(np.uint64)), key
        else:
            assert np.array_equal(a[key], b[key]), key


def test_fit_device_equals_fit_np_in_one_chunk_and_in_chunks_of_two():
    scans, Ts, ids, options = RO.cases()['ragged']
    want = road_fit.fit_np(scans, Ts, ids, **options)
    assert want['valid'].sum() >= 2 and not want['valid'].all()
    whole = road_fit.fit_device(scans, Ts, ids, **options)
    same_fit(whole, want)
    parts = [road_fit.fit_device(scans[a:a + 2], Ts[a:a + 2], ids[a:a + 2], **options) for a in (0, 2, 4)]
    same_fit({k: np.concatenate([p[k] for p in parts]) for k in whole}, want)


def test_a_second_run_returns_the_same_bytes():
    scans, Ts, ids, options = RO.cases()['ragged']
    first = road_fit.device_stages(scans, Ts, ids, **options)
    second = road_fit.device_stages(scans, Ts, ids, **options)
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
    a, b = road_fit.fit_device(scans, Ts, ids, **options), road_fit.fit_device(scans, Ts, ids, **options)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_exact_recovery_on_the_device():
    case, truth, on_plane = RO.exact_case()
    got = road_fit.fit_device(*case[:3], **case[3])
    assert got['inliers'][0] == on_plane and got['winner'][0] == RO.expected('exact')['winner'][0]
    assert np.abs(got['planes'][0] - truth).max() <= 1e-12


def test_argument_errors_launch_nothing():
    lib = hip.lib()
    dev = 'cuda'
    pts = torch.zeros((16, 4), dtype=torch.float32, device=dev)
    off = torch.tensor([0, 16], dtype=torch.int32, device=dev)
    T = torch.zeros((1, 12), dtype=torch.float64, device=dev)
    ids = torch.zeros((1,), dtype=torch.int32, device=dev)
    q = torch.full((16, 3), 7, dtype=torch.int32, device=dev)
    kept = torch.full((1,), 7, dtype=torch.int32, device=dev)
    count = torch.full((1, 8), 7, dtype=torch.int32, device=dev)
    winner = torch.full((1,), 7, dtype=torch.int32, device=dev)
    inliers = torch.full((1,), 7, dtype=torch.int32, device=dev)
    sums = torch.full((1, 10), 7, dtype=torch.int64, device=dev)
    p, st = hip.ptr, hip.stream_ptr()

    def points(F=1, total=16, mp=16, xq=5120, yq=2048, zq=12800, src=pts.data_ptr(), out=q.data_ptr()):
        return lib.gpp_road_points_i32(ctypes.c_void_p(src), p(off), p(T), F, total, mp, xq, yq, zq, ctypes.c_void_p(out), p(kept), st)
    assert points(xq=10241) == -1 and points(yq=2049) == -1 and points(zq=20481) == -1 and points(zq=0) == -1 and points(xq=-1) == -1
    assert points(F=-1) == -1 and points(F=65536) == -1 and points(mp=17) == -1 and points(mp=(1 << 20) + 1, total=1 << 21) == -1
    assert points(out=None) == -1 and points(src=None) == -1 and points(src=pts.data_ptr() + 4) == -3 and points(F=0) == 0

    def score(F=1, H=8, c2=0.9, hlo2=1.0, hhi2=2.0, tq2=3.0, out=count.data_ptr()):
        return lib.gpp_road_score(p(q), p(off), p(kept), p(ids), 0, F, 16, 16, H, c2, hlo2, hhi2, tq2, ctypes.c_void_p(out), st)
    nan = float('nan')
    assert score(H=-1) == -1 and score(H=(1 << 20) + 1) == -1 and score(c2=1.5) == -1 and score(c2=nan) == -1 and score(hlo2=3.0) == -1
    assert score(tq2=-1.0) == -1 and score(tq2=nan) == -1 and score(out=None) == -1 and score(H=0) == 0 and score(F=0) == 0
    assert lib.gpp_road_winner(p(count), 1, 8, 0, p(winner), p(inliers), st) == -1
    assert lib.gpp_road_winner(p(count), 1, 8, 5, None, p(inliers), st) == -1 and lib.gpp_road_winner(None, 1, 8, 5, p(winner), p(inliers), st) == -1
    assert lib.gpp_road_moments(p(q), p(off), p(kept), p(ids), 0, p(winner), 1, 16, 16, 8, nan, p(sums), st) == -1
    assert lib.gpp_road_moments(p(q), p(off), p(kept), p(ids), 0, None, 1, 16, 16, 8, 1.0, p(sums), st) == -1
    assert lib.gpp_road_moments(p(q), p(off), p(kept), p(ids), 0, p(winner), 1, 16, 16, 8, 1.0, ctypes.c_void_p(sums.data_ptr() + 4), st) == -3
    torch.cuda.synchronize()
    for t in (q, kept, count, winner, inliers, sums):
        assert (t == 7).all()
    with pytest.raises(ValueError):
        hip.road_points(pts, off, T.reshape(12), 16, (5120, 2048, 12800))
    # offsets that descend or leave the batch: an empty frame to every launch, nothing outside the batch is touched
    bad = torch.tensor([0, 12, 4, 40, 16], dtype=torch.int32, device=dev)
    cam = RO.dyadic_plane_cloud(np.random.default_rng(1), 16, 1.5)
    pts2 = torch.as_tensor(RO.to_velodyne(cam)).to(dev)
    T4 = torch.as_tensor(np.tile(RO.PERMUTE.reshape(1, 12), (4, 1))).to(dev)
    q2, kept2 = hip.road_points(pts2, bad, T4, 16, (5120, 2048, 12800))
    ids4 = torch.zeros((4,), dtype=torch.int32, device=dev)
    count2 = hip.road_score(q2, bad, kept2, ids4, 0, 16, 8, 0.9, 256.0 ** 2, 640.0 ** 2, 25.6 ** 2)
    winner2, inliers2 = hip.road_winner(count2, 3)
    sums2 = hip.road_moments(q2, bad, kept2, ids4, 0, winner2, 16, 8, 25.6 ** 2)
    torch.cuda.synchronize()
    assert kept2.tolist() == [12, 0, 0, 0] and (count2[1:] == -1).all() and (winner2[1:] == -1).all() and not sums2[1:].any()
    assert not q2[12:].any() and inliers2[0] == 12 and sums2[0][0] == 12


# ---------------------------------------------------------------------------------------------------- through the rest of the project
def own_plane_scenes():
    """ five images of eight Cars, each on a horizontal dyadic plane of its own: y = 1.25 + k / 64, k = 0 .. 39 """
    scenes, planes = [], []
    for b, seed in enumerate((31, 32, 33, 34, 35)):
        labels, P = LO.seeded_scene(seed, 8, P_offset=False, kinds=(0,), behind=0.0)
        labels[:, 12] = 1.25 + (8 * b + np.arange(8)) / 64.0
        planes += [[0.0, -1.0, 0.0, t] for t in labels[:, 12]]
        scenes.append((['Car'] * 8, labels, P))
    return scenes, np.array(planes, np.float64)


def write_scans(root, scans, Ts):
    velo, calib = os.path.join(str(root), 'velodyne'), os.path.join(str(root), 'velo_calib')
    os.makedirs(velo), os.makedirs(calib)
    for i, (p, T) in enumerate(zip(scans, Ts)):
        np.asarray(p, np.float32).tofile(os.path.join(velo, '%06d.bin' % i))
        with open(os.path.join(calib, '%06d.txt' % i), 'w') as f:
            f.write('R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: ' + ' '.join(repr(float(v)) for v in np.asarray(T).ravel()) + '\n')
    return velo, calib


def test_scans_to_pool_to_database_to_polling(tmp_path, capsys):
    scenes, own = own_plane_scenes()
    rng = np.random.default_rng(3)
    scans = [RO.to_velodyne(RO.dyadic_plane_cloud(rng, 400, t)) for t in own[:, 3]]       # one noise-free cloud per plane
    velo, calib = write_scans(tmp_path, scans, [RO.PERMUTE] * 40)
    pool = road_fit.fit_pool(velo, calib, chunk_frames=16, hypotheses=64)
    assert pool['record']['valid'].all() and (pool['record']['inliers'] == 400).all() and len(pool['files']) == 40
    assert np.array_equal(pool['planes'], own)               # dyadic planes, exact sums: the fit returns them to the bit
    same_fit(pool['record'], road_fit.fit_np(scans, [RO.PERMUTE] * 40, list(range(40)), hypotheses=64))
    labels_list, P_list = [g for _, g, _ in scenes], [P for _, _, P in scenes]
    on_truth = plane_db.distil_rows(labels_list, P_list, own, 40)
    fitted = plane_db.distil_rows(labels_list, P_list, pool['planes'], 40)
    assert on_truth['six_vote_share'] == 1.0 and fitted['six_vote_share'] == 1.0 and fitted['served'] == fitted['objects'] >= 30
    assert np.array_equal(fitted['indices'], on_truth['indices'])
    # the command line writes the same pool, which the rest of the project reads back
    out = os.path.join(str(tmp_path), 'pool.mat')
    result = fit_plane_pool.main([velo, calib, out, '--hypotheses', '64'])
    assert '40 frames, 40 valid' in capsys.readouterr().out and np.array_equal(result['planes'], pool['planes'])
    assert np.array_equal(L._load_planes(out), own.astype(np.float32))
