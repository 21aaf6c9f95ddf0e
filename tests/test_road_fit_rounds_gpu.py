""" Several road planes per frame on the GPU (csrc/road_fit.hip gpp_road_peel_i32): the peel against its NumPy form
(road_fit.peel_np) and the loop-written oracle (tests/road_fit_rounds_oracle.py) with winners from the real pipeline and hand-set ones, on
the smallest frames at which each part of the kernel can go wrong; every stage of every round of the whole fit; and the chain
scans -> pool -> database -> polling, which needs two planes per frame to serve every object.

Every comparison is for equality: the fit is integer arithmetic and documented single float64 operations. """
import ctypes
import os

import numpy as np
import pytest
import torch

import label_prep_oracle as LO
import road_fit_oracle as RO
import road_fit_rounds_oracle as RR
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.bin import fit_plane_pool
from keras_retinanet_3D.utils import plane_db, road_fit
from keras_retinanet_3D.utils import label_prep as L

pytestmark = pytest.mark.gpu

BLOCK = 2048                                                  # GPP_ROAD_PEEL_BLOCK (include/gpp.h)
PATTERN = 0x5a5a5a5a
SIZES = (0, 1, 3, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
DEV = 'cuda'


def up(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def level_cloud(rng, m, share=0.6):
    """ m quantised points (m, 3) int32: `share` of them on y = 1.5 m (dyadic: exact), the others up to 1 m above, in a random order """
    cam = RO.dyadic_plane_cloud(rng, m, 1.5)
    off = rng.random(m) >= share
    cam[off, 1] -= rng.integers(30, 257, int(off.sum())) / 256.0
    return np.round(cam * 256.0).astype(np.int32)


def batch_of(frames, gaps):
    """ frames: a list of (m, 3) int32 kept points; gaps: rows owned by the frame behind its kept points (filled with a pattern, as the rows
    that gpp_road_points_i32 leaves behind a frame's kept points) -> (q (total, 3), offsets (F + 1,), kept (F,)) """
    rows, offsets = [], [0]
    for v, g in zip(frames, gaps):
        rows += [v, np.full((g, 3), 0x7f7f7f7f, np.int32)]
        offsets.append(offsets[-1] + v.shape[0] + g)
    return np.concatenate(rows).astype(np.int32), np.asarray(offsets, np.int32), np.asarray([v.shape[0] for v in frames], np.int32)


def peel_on_device(q, offsets, kept, ids, seed, winner, H, tq2):
    """ hip.road_peel (its q_out starts as zeros), and gpp_road_moments for the same winner -> (q_out, kept_out, sums) as arrays """
    mp = int(np.diff(offsets).max())
    q_d, off_d, kept_d, ids_d, win_d = up(q), up(offsets), up(kept), up(np.asarray(ids, np.uint32).view(np.int32)), up(np.asarray(winner, np.int32))
    q_out, kept_out = hip.road_peel(q_d, off_d, kept_d, ids_d, seed, win_d, mp, H, tq2)
    sums = hip.road_moments(q_d, off_d, kept_d, ids_d, seed, win_d, mp, H, tq2)
    torch.cuda.synchronize()
    assert np.array_equal(q_d.cpu().numpy(), q)              # the input is not changed
    return q_out.cpu().numpy(), kept_out.cpu().numpy(), sums.cpu().numpy()


def check_peel(frames, gaps, ids, seed, winner, o, oracle=True):
    """ the device peel of a batch against peel_np (and the loop oracle): survivors row for row in their order, zeros behind them in the
    frame's segment, kept_in - kept_out == N of gpp_road_moments """
    q, offsets, kept = batch_of(frames, gaps)
    orr = dict(o, seed=seed)
    got_q, got_kept, sums = peel_on_device(q, offsets, kept, ids, seed, winner, o['H'], o['tq2'])
    for f, v in enumerate(frames):
        want = road_fit.peel_np(v, ids[f], int(winner[f]), orr)
        a, b = int(offsets[f]), int(offsets[f + 1])
        assert got_kept[f] == want.shape[0], f
        assert np.array_equal(got_q[a:a + want.shape[0]], want), f
        assert not got_q[a + want.shape[0]:b].any(), f
        if oracle:
            pts = [tuple(p) for p in v.tolist()]
            assert [tuple(p) for p in want.tolist()] == RR.peel(pts, ids[f], int(winner[f]), orr), f
            assert sums[f, 0] == RR.inlier_count(pts, ids[f], int(winner[f]), orr), f
        if 0 <= winner[f] < o['H']:
            assert kept[f] - got_kept[f] == sums[f, 0], f
    return got_q, got_kept, sums


def pipeline_winner(frames, gaps, ids, seed, o):
    q, offsets, kept = batch_of(frames, gaps)
    mp = int(np.diff(offsets).max())
    q_d, off_d, kept_d, ids_d = up(q), up(offsets), up(kept), up(np.asarray(ids, np.uint32).view(np.int32))
    count = hip.road_score(q_d, off_d, kept_d, ids_d, seed, mp, o['H'], o['c2'], o['hlo2'], o['hhi2'], o['tq2'])
    winner, _ = hip.road_winner(count, o['min_inliers'])
    return winner.cpu().numpy()


@pytest.fixture(scope='module')
def ragged():
    rng = np.random.default_rng(24)
    frames = [level_cloud(rng, m) for m in SIZES]
    gaps = [int(g) for g in rng.integers(0, 70, len(SIZES))]
    return frames, gaps, [int(v) for v in rng.integers(0, 1 << 32, len(SIZES))]


def test_peel_of_a_ragged_batch_with_the_pipelines_winners(ragged):
    frames, gaps, ids = ragged
    o = road_fit.resolve_options(hypotheses=48, min_inliers=2)
    seed = road_fit.round_seed(11, 1)
    winner = pipeline_winner(frames, gaps, ids, seed, o)
    assert (winner[:2] == -1).all() and (winner[3:] >= 0).all()
    _, kept_out, _ = check_peel(frames, gaps, ids, seed, winner, o)
    assert (kept_out[3:] > 0).all() and (kept_out[3:] < np.asarray(SIZES[3:])).all() and not kept_out[:2].any()


@pytest.mark.parametrize('h', [0, 17, 47, -1])
def test_peel_of_a_ragged_batch_with_hand_set_winners(ragged, h):
    frames, gaps, ids = ragged
    o = road_fit.resolve_options(hypotheses=48, min_inliers=2)
    winner = np.full(len(frames), h, np.int32)
    if h == 17:
        winner = ((np.arange(len(frames)) * 7 + 3) % 48).astype(np.int32)
        winner[5] = -1
    _, kept_out, _ = check_peel(frames, gaps, ids, 0xfffffff0, winner, o)
    if h == -1:
        assert not kept_out.any()


def gated_scans():
    """ scans whose kept counts are SIZES, each with 40 gated-out points between the kept ones (as road_fit_oracle._slab): the kept points'
    positions in the scan differ from their positions in q """
    rng = np.random.default_rng(29)
    scans = []
    for m in SIZES:
        cam = level_cloud(rng, m) / 256.0
        outside = RO.road_cloud(rng, 40)
        outside[:, 0] += 60.0
        both = np.concatenate([cam, outside])
        order = np.argsort(np.concatenate([np.arange(m) * 2.0, rng.uniform(0, max(1, 2 * m), 40)]), kind='stable')
        scans.append(RO.to_velodyne(both[order]))
    return scans, [RO.PERMUTE] * len(SIZES), list(range(100, 100 + len(SIZES))), dict(hypotheses=48, min_inliers=2, seed=7)


def test_peel_behind_the_gate_on_scans_with_gated_out_points_between_the_kept_ones():
    scans, Ts, ids, options = gated_scans()
    o = road_fit.resolve_options(**options)
    got = road_fit.device_round_stages(scans, Ts, ids, 2, **options)
    host = road_fit.np_round_stages(scans, Ts, ids, 2, **options)
    want = RR.rounds(scans, Ts, ids, 2, **options)
    assert got[0]['kept'].tolist() == list(SIZES) and (got[0]['winner'][3:] >= 0).all()
    for r in range(2):
        w = RR.as_arrays(want[r], o['H'])
        for key in ('kept', 'count', 'winner', 'inliers', 'sums'):
            assert np.array_equal(got[r][key], w[key]) and np.array_equal(got[r][key], host[r][key]), (r, key)
        for f in range(len(scans)):
            a, b, m = int(got[r]['offsets'][f]), int(got[r]['offsets'][f + 1]), int(w['kept'][f])
            assert b - a == SIZES[f] + 40
            assert [tuple(p) for p in got[r]['q'][a:a + m].tolist()] == want[r]['q'][f], (r, f)
            assert not got[r]['q'][a + m:b].any(), (r, f)
    has = got[0]['winner'] >= 0
    assert np.array_equal((got[0]['kept'] - got[1]['kept'])[has], got[0]['sums'][has, 0]) and (got[1]['kept'][3:] > 0).all()


def test_peel_of_a_frame_with_more_blocks_than_the_scan_has_lanes():
    """ 256 . 2048 + 5 kept points: 257 block counts, the scan workgroup's second chunk; H = 3.  Against peel_np; the loop oracle gets the
    3 . 2048 + 7 cousin """
    rng = np.random.default_rng(25)
    o = road_fit.resolve_options(hypotheses=3, min_inliers=2)
    big = level_cloud(rng, 256 * BLOCK + 5, share=0.5)
    winner = pipeline_winner([big], [0], [9], 5, o)
    assert winner[0] >= 0
    _, kept_out, _ = check_peel([big], [0], [9], 5, winner, o, oracle=False)
    assert 0 < kept_out[0] < 256 * BLOCK + 5
    cousin = level_cloud(rng, 3 * BLOCK + 7, share=0.5)
    frames, gaps, ids = [cousin, cousin[:5]], [3, 0], [9, 10]
    winner = pipeline_winner(frames, gaps, ids, 5, o)
    assert winner[0] >= 0
    check_peel(frames, gaps, ids, 5, winner, o)


def test_peel_where_every_point_goes_and_where_only_coplanar_points_go():
    rng = np.random.default_rng(26)
    o = road_fit.resolve_options(hypotheses=16, min_inliers=2)
    flat = level_cloud(rng, BLOCK + 300, share=1.1)           # every point on the plane
    winner = pipeline_winner([flat], [5], [3], 1, o)
    _, kept_out, sums = check_peel([flat], [5], [3], 1, winner, o)
    assert winner[0] >= 0 and kept_out[0] == 0 and sums[0, 0] == BLOCK + 300
    # tq2 = 0: only points exactly on the winner's plane go -- the three drawn ones and the few exactly coplanar ones
    cloud = np.stack([rng.integers(-5000, 5001, 700), rng.integers(200, 600, 700), rng.integers(300, 12000, 700)], axis=1).astype(np.int32)
    o0 = dict(o, tq2=0.0)
    draws = road_fit.draw_indices(1, 4, 16, 700)[2].tolist()
    assert len(set(draws)) == 3
    p0, u, v = np.array([0, 400, 6000]), np.array([700, 3, 100]), np.array([-200, -2, 900])
    cloud[draws[0]], cloud[draws[1]], cloud[draws[2]] = p0, p0 + 2 * u, p0 + 2 * v
    spare = [i for i in range(700) if i not in draws]
    for k, (i, j) in enumerate(((1, 0), (0, 1), (1, 1), (2, 2))):        # exactly coplanar: p0 + i u + j v
        cloud[spare[k * 50]] = p0 + i * u + j * v
    on = ((cloud.astype(np.int64) - p0) @ np.cross(2 * u, 2 * v) == 0)
    assert 7 <= on.sum() <= 9                                 # the three drawn points, the four made ones (and a chance point at the most)
    winner = np.array([2], np.int32)
    got_q, kept_out, sums = check_peel([cloud], [0], [4], 1, winner, o0)
    assert kept_out[0] == 700 - on.sum() and np.array_equal(got_q[:kept_out[0]], cloud[~on])


def test_peel_with_a_winner_whose_draws_repeat_a_point():
    """ three kept points: most hypotheses draw one of them twice, n = 0.  Hand-set as the winner such a hypothesis has no inliers, for
    gpp_road_moments and for the peel alike """
    rng = np.random.default_rng(27)
    o = road_fit.resolve_options(hypotheses=32, min_inliers=1)
    three, more = level_cloud(rng, 3), level_cloud(rng, 300)
    draws = road_fit.draw_indices(8, 1, 32, 3)
    h0 = next(h for h in range(32) if len(set(draws[h].tolist())) < 3)
    h1 = next(h for h in range(32) if len(set(draws[h].tolist())) == 3)
    for h in (h0, h1):
        winner = np.array([h, 5], np.int32)
        _, kept_out, sums = check_peel([three, more], [4, 0], [1, 2], 8, winner, o)
        assert kept_out[0] == (3 if h == h0 else 0) and sums[0, 0] == 3 - kept_out[0]
    two = check_peel([three[:2], three[:1]], [1, 1], [1, 2], 8, np.array([h1, h1], np.int32), o)      # fewer than three points: no plane
    assert two[1].tolist() == [2, 1] and not two[2].any()


def raw_peel(lib, q_in, off, kept, ids, winner, F, total, mp, H, tq2, q_out, kept_out, ws, ws_bytes, seed=0):
    c = lambda v: v if v is None or isinstance(v, ctypes.c_void_p) else hip.ptr(v)  # noqa: E731
    return lib.gpp_road_peel_i32(c(q_in), c(off), c(kept), c(ids), seed, c(winner), F, total, mp, H, tq2, c(q_out), c(kept_out), c(ws), ws_bytes,
                                 hip.stream_ptr())


def test_bad_offsets_are_empty_frames_and_nothing_else_is_touched():
    rng = np.random.default_rng(28)
    lib = hip.lib()
    o = road_fit.resolve_options(hypotheses=8, min_inliers=2)
    a, b = level_cloud(rng, 300), level_cloud(rng, 100)
    q = np.concatenate([a, np.full((20, 3), 0x7f7f7f7f, np.int32), b]).astype(np.int32)        # total 420
    F, total, mp = 6, 420, 320

    def run(off, kept, winner):
        q_d, off_d, kept_d, win_d = up(q), up(off), up(kept), up(winner)
        ids_d = up(np.arange(F, dtype=np.int32))
        q_out = torch.full((total + 64, 3), PATTERN, dtype=torch.int32, device=DEV)           # 32 guard rows on either side
        kept_out = torch.full((F,), PATTERN, dtype=torch.int32, device=DEV)
        need = ctypes.c_size_t(0)
        assert lib.gpp_road_peel_workspace_bytes(F, mp, ctypes.byref(need)) == 0
        ws = torch.zeros((need.value,), dtype=torch.uint8, device=DEV)
        rc = raw_peel(lib, q_d, off_d, kept_d, ids_d, win_d, F, total, mp, o['H'], o['tq2'], ctypes.c_void_p(q_out.data_ptr() + 32 * 12), kept_out, ws,
                      need.value)
        torch.cuda.synchronize()
        assert rc == 0
        return q_out.cpu().numpy(), kept_out.cpu().numpy()

    # frames are consecutive in `offsets`, so one bad number breaks two frames; F = 6 frames over the 420 rows, max_points = 320
    chains = (([0, 320, 100, 320, 420, 420, 420], [300, 50, 0, 100, 0, 0]),       # frame 1 = (320, 100) descends; frame 2 lies over frame 0's rows: kept 0
              ([0, 320, 100, 500, 420, 420, 420], [300, 50, 50, 100, 7, 0]),      # frame 2 = (100, 500) leaves the batch, frame 3 = (500, 420) descends
              ([0, 320, 320, 320, 0, 420, 420], [300, 0, 0, 100, 50, 0]),         # frame 3 = (320, 0) descends, frame 4 = (0, 420) spans more than max_points
              ([0, 320, 320, 320, 420, -4, 40], [300, 0, 0, 100, 3, 20]))         # frame 4 = (420, -4) descends, frame 5 = (-4, 40) starts before the batch
    winner = np.array([1, 2, 2, 3, 2, 2], np.int32)
    for bad, (chain, kept) in enumerate(chains):
        kept = np.asarray(kept, np.int32)
        chain = np.asarray(chain, np.int32)
        got_q, got_kept = run(chain, kept, winner)
        assert (got_q[:32] == PATTERN).all() and (got_q[32 + total:] == PATTERN).all()
        body = got_q[32:32 + total]
        orr = dict(o, seed=0)
        touched = np.zeros(total, bool)
        for f in range(F):
            lo, hi = int(chain[f]), int(chain[f + 1])
            ok = lo >= 0 and hi >= lo and hi <= total and hi - lo <= mp
            if not ok:
                assert got_kept[f] == 0, (bad, f)
                continue
            m = min(max(int(kept[f]), 0), hi - lo)
            want = road_fit.peel_np(q[lo:lo + m], f, int(winner[f]), orr)
            assert got_kept[f] == want.shape[0] and np.array_equal(body[lo:lo + want.shape[0]], want), (bad, f)
            touched[lo:lo + want.shape[0]] = True
        assert (body[~touched] == PATTERN).all(), bad


def test_argument_errors_launch_nothing():
    lib = hip.lib()
    q = torch.full((16, 3), 7, dtype=torch.int32, device=DEV)
    big = torch.full((40, 3), 7, dtype=torch.int32, device=DEV)
    q_out = torch.full((16, 3), 7, dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 16], dtype=torch.int32, device=DEV)
    kept = torch.full((1,), 16, dtype=torch.int32, device=DEV)
    ids = torch.zeros((1,), dtype=torch.int32, device=DEV)
    winner = torch.zeros((1,), dtype=torch.int32, device=DEV)
    kept_out = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    need = ctypes.c_size_t(0)
    assert lib.gpp_road_peel_workspace_bytes(1, 16, ctypes.byref(need)) == 0 and need.value >= 4
    assert lib.gpp_road_peel_workspace_bytes(1, 16, None) == -1 and lib.gpp_road_peel_workspace_bytes(-1, 16, ctypes.byref(need)) == -1
    assert lib.gpp_road_peel_workspace_bytes(65536, 16, ctypes.byref(need)) == -1
    assert lib.gpp_road_peel_workspace_bytes(1, (1 << 20) + 1, ctypes.byref(need)) == -1 and lib.gpp_road_peel_workspace_bytes(1, -1, ctypes.byref(need)) == -1
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gpp_road_peel_workspace_bytes(3, 2048, ctypes.byref(a)) == 0 and lib.gpp_road_peel_workspace_bytes(3, 2049, ctypes.byref(b)) == 0
    assert b.value - a.value == 3 * 4                        # one more block count per frame
    assert lib.gpp_road_peel_workspace_bytes(1, 16, ctypes.byref(need)) == 0
    ws = torch.full((need.value + 8,), 7, dtype=torch.uint8, device=DEV)
    vp = ctypes.c_void_p

    def peel(F=1, total=16, mp=16, H=8, tq2=1.0, src=q, dst=q_out, o=off, k=kept, i=ids, w=winner, ko=kept_out, work=ws, nbytes=need.value):
        return raw_peel(lib, src, o, k, i, w, F, total, mp, H, tq2, dst, ko, work, nbytes)
    nan = float('nan')
    assert peel(F=-1) == -1 and peel(F=65536) == -1 and peel(mp=17) == -1 and peel(total=-1) == -1 and peel(mp=(1 << 20) + 1, total=1 << 21) == -1
    assert peel(H=-1) == -1 and peel(H=(1 << 20) + 1) == -1 and peel(tq2=nan) == -1 and peel(tq2=-1.0) == -1
    assert peel(src=None) == -1 and peel(dst=None) == -1 and peel(o=None) == -1 and peel(k=None) == -1 and peel(i=None) == -1
    assert peel(w=None) == -1 and peel(ko=None) == -1 and peel(work=None) == -1
    assert peel(dst=q) == -1                                  # q_out == q_in
    assert peel(src=big, dst=vp(big.data_ptr() + 15 * 12)) == -1 and peel(src=vp(big.data_ptr() + 15 * 12), dst=big) == -1      # overlapping ranges
    assert peel(src=vp(big.data_ptr() + 4), dst=vp(big.data_ptr() + 4 + 16 * 12 - 4)) == -1
    assert peel(nbytes=need.value - 1) == -2                  # a workspace one byte short
    assert peel(dst=vp(big.data_ptr() + 2)) == -3 and peel(src=vp(big.data_ptr() + 1)) == -3 and peel(ko=vp(kept_out.data_ptr() + 2)) == -3
    assert peel(work=vp(ws.data_ptr() + 1)) == -3
    assert peel(F=0) == 0 and peel(F=0, src=None, dst=None, work=None, nbytes=0) == 0
    torch.cuda.synchronize()
    for t in (q, big, q_out, kept_out, ws):
        assert (t == 7).all()
    # two buffers side by side in one allocation are no overlap: this one launches
    assert peel(src=big, dst=vp(big.data_ptr() + 16 * 12)) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        hip.road_peel(q, off, kept, ids, 0, winner.reshape(1, 1), 16, 8, 1.0)


# ---------------------------------------------------------------------------------------------------- every stage of every round
def case(name):
    return RR.two_level_frames() if name == 'two_level' else RO.cases()[name]


@pytest.fixture(scope='module')
def round_stages():
    return {name: road_fit.device_round_stages(*case(name)[:3], 3, **case(name)[3]) for name in ('two_level', 'ragged')}


@pytest.mark.parametrize('name', ['two_level', 'ragged'])
def test_every_stage_of_every_round_equals_numpy_and_the_oracle(round_stages, name):
    scans, Ts, ids, options = case(name)
    o = road_fit.resolve_options(**options)
    got, host, want = round_stages[name], road_fit.np_round_stages(scans, Ts, ids, 3, **options), RR.expected_rounds(name)
    for r in range(3):
        w = RR.as_arrays(want[r], o['H'])
        for key in ('kept', 'count', 'winner', 'inliers', 'sums'):
            assert got[r][key].dtype == w[key].dtype and np.array_equal(got[r][key], w[key]), (r, key)
            assert np.array_equal(got[r][key], host[r][key]), (r, key)
        for f in range(len(scans)):
            a, b, m = int(got[r]['offsets'][f]), int(got[r]['offsets'][f + 1]), int(w['kept'][f])
            assert [tuple(p) for p in got[r]['q'][a:a + m].tolist()] == want[r]['q'][f], (r, f)
            assert np.array_equal(got[r]['q'][a:a + m], host[r]['q'][f]) and not got[r]['q'][a + m:b].any(), (r, f)
    for r in range(2):
        has = got[r]['winner'] >= 0
        assert has.any() and np.array_equal((got[r]['kept'] - got[r + 1]['kept'])[has], got[r]['sums'][has, 0])


def same_fit(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        if a[key].dtype == np.float64:
            assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])), key
            assert np.array_equal(a[key][~np.isnan(a[key])].view(np.uint64), b[key][~np.isnan(b[key])].view(np.uint64)), key
        else:
            assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize('name', ['two_level', 'ragged'])
def test_fit_rounds_device_in_one_chunk_in_chunks_of_two_and_again(round_stages, name):
    scans, Ts, ids, options = case(name)
    want = road_fit.fit_rounds_np(scans, Ts, ids, 3, **options)
    whole = road_fit.fit_rounds_device(scans, Ts, ids, 3, **options)
    same_fit(whole, want)
    parts = [road_fit.fit_rounds_device(scans[a:a + 2], Ts[a:a + 2], ids[a:a + 2], 3, **options) for a in range(0, len(scans), 2)]
    same_fit({k: np.concatenate([p[k] for p in parts]) for k in whole}, want)
    again = road_fit.device_round_stages(scans, Ts, ids, 3, **options)
    for r in range(3):
        for key in again[r]:
            assert again[r][key].tobytes() == round_stages[name][r][key].tobytes(), (r, key)
    one = road_fit.fit_device(scans, Ts, ids, **options)     # round 0 is today's fit
    for key in one:
        assert np.ascontiguousarray(whole[key][:, 0]).tobytes() == one[key].tobytes(), key


# ---------------------------------------------------------------------------------------------------- through the rest of the project
def two_level_scenes():
    """ five images of eight Cars: Car j of image b stands on plane 8 b + j of the 40 true planes in (frame, round) order """
    truth = RR.two_level_truth()
    scenes = []
    for b, seed in enumerate((31, 32, 33, 34, 35)):
        labels, P = LO.seeded_scene(seed, 8, P_offset=False, kinds=(0,), behind=0.0)
        labels[:, 12] = truth[8 * b:8 * b + 8, 3]
        scenes.append((['Car'] * 8, labels, P))
    return scenes, truth


def write_scans(root, scans, Ts):
    velo, calib = os.path.join(str(root), 'velodyne'), os.path.join(str(root), 'velo_calib')
    os.makedirs(velo), os.makedirs(calib)
    for i, (p, T) in enumerate(zip(scans, Ts)):
        np.asarray(p, np.float32).tofile(os.path.join(velo, '%06d.bin' % i))
        with open(os.path.join(calib, '%06d.txt' % i), 'w') as f:
            f.write('R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: ' + ' '.join(repr(float(v)) for v in np.asarray(T).ravel()) + '\n')
    return velo, calib


def test_two_planes_per_frame_serve_every_object(tmp_path, capsys):
    scenes, truth = two_level_scenes()
    scans, Ts, ids, options = RR.two_level_frames()
    velo, calib = write_scans(tmp_path, scans, Ts)
    pool = road_fit.fit_pool(velo, calib, chunk_frames=8, planes_per_frame=2, hypotheses=64)
    assert np.array_equal(pool['planes'], truth) and pool['rounds'].tolist() == [0, 1] * 20
    assert pool['files'] == [n for i in range(20) for n in ['%06d.bin' % i] * 2]
    same_fit(pool['record'], road_fit.fit_rounds_np(scans, Ts, ids, 2, hypotheses=64))
    labels_list, P_list = [g for _, g, _ in scenes], [P for _, _, P in scenes]
    on_truth = plane_db.distil_rows(labels_list, P_list, truth, 40)
    fitted = plane_db.distil_rows(labels_list, P_list, pool['planes'], 40)
    assert on_truth['six_vote_share'] == 1.0 and fitted['six_vote_share'] == 1.0 and fitted['served'] == fitted['objects'] == 40
    assert np.array_equal(fitted['indices'], on_truth['indices'])
    # one plane per frame: half of the Cars stand on a level that the pool does not hold
    single = road_fit.fit_pool(velo, calib, chunk_frames=8, hypotheses=64)
    assert single['planes'].shape == (20, 4) and np.array_equal(single['planes'], truth[0::2])
    assert plane_db.distil_rows(labels_list, P_list, single['planes'], 20)['six_vote_share'] < 1.0
    # the command line writes the same pool, which the rest of the project reads back
    out = os.path.join(str(tmp_path), 'pool.mat')
    result = fit_plane_pool.main([velo, calib, out, '--hypotheses', '64', '--planes-per-frame', '2'])
    assert '20 frames, 20 valid, 40 planes' in capsys.readouterr().out and np.array_equal(result['planes'], pool['planes'])
    assert np.array_equal(L._load_planes(out), truth.astype(np.float32))
