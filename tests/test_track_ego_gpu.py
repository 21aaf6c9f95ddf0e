""" GPU tests of the tracker's ego-motion compensation (csrc/track.hip, gpp_track_ego_f64): the kernel against the
NumPy form (utils/track.py) and the loop-written oracle (tests/track_ego_oracle.py) on the cases of tests/test_track_ego_cpu.py, which
asserts their margins, for both assignments; the curve through the plain entry point and through the new one in one process; chunked
calls, several sequences in one call, in place; one full case; the contract's errors; RetinaNet3D(pose=True, track={..., 'ego': True})
end to end, and a model without 'ego' after it. """
import ctypes

import numpy as np
import pytest
import torch

import track_ego_oracle as E
import track_optimal_oracle as P
import track_oracle as O
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import synthetic
from keras_retinanet_3D.utils import track as T

pytestmark = pytest.mark.gpu

EXACT = E.exact_cases()
MARGIN = E.margin_cases()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def alpha_within_4_ulp(got, want):
    """ column 25 of smoothed rows: 4 float32 ulp of the oracle's value (the bar of tests/test_track_gpu.py); bit-equal elsewhere """
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    return bool((same | (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 4 * np.spacing(np.abs(want)).astype(np.float64))).all())


def rows_agree(got, want, smooth):
    cols = [c for c in range(36) if c != 25 or not smooth]
    return same_bytes(got[..., cols], want[..., cols]) and alpha_within_4_ulp(got[..., 25], want[..., 25])


def rows_equal(got, want, smooth):
    """ against the oracle, whose placement around the imported step may change a zero's sign (its docstring): ==, not bytes """
    cols = [c for c in range(36) if c != 25 or not smooth]
    return np.array_equal(got[..., cols], want[..., cols], equal_nan=True) and alpha_within_4_ulp(got[..., 25], want[..., 25])


def option(metric, thr=None, assign='greedy', **more):
    opt = O.options(metric, thr, **more)
    return P.optimal(opt) if assign == 'optimal' else opt


@pytest.mark.parametrize('name,frames,ego,opt', EXACT + MARGIN, ids=[c[0] for c in EXACT + MARGIN])
def test_kernel_equals_the_host_form_and_the_oracle(name, frames, ego, opt):
    """ ids, hits and every state field: ==.  Signed permutations with dyadic numbers, or the margins that tests/test_track_ego_cpu.py
    asserts """
    o_rows, o_ids, o_hits, o_state = E.track(frames, opt, ego)
    n_rows, n_ids, n_hits, n_state = T.track_rows_np(frames, opt, ego=ego)
    rows, ids, hits, state = T.track_rows_device(frames, opt, ego=ego)
    assert rows.dtype == np.float32 and ids.dtype == np.int32 and hits.dtype == np.int32 and rows.shape == frames.shape
    assert np.array_equal(ids, n_ids) and np.array_equal(ids, o_ids)
    assert np.array_equal(hits, n_hits) and np.array_equal(hits, o_hits)
    assert same_bytes(state, n_state) and O.same_state(o_state, state)
    assert rows_equal(rows, o_rows, opt['smooth']) and rows_agree(rows, n_rows, opt['smooth'])
    if not opt['smooth']:
        assert same_bytes(rows, frames)


@pytest.mark.parametrize('assign', T.ASSIGNS)
def test_the_curve_through_both_entry_points_in_one_process(assign):
    """ 8 parked cars, 12 frames, 1.5 m and 0.04 rad of ego-motion per frame: the plain entry point tears the tracks, the new one keeps
    one id per car """
    frames, ego, gts = E.curve()
    for metric, thr in E.FOR:
        opt = option(metric, thr, assign)
        _, plain_ids, _, plain_state = T.track_rows_device(frames, opt)
        assert int(plain_state['next_id']) > E.CARS and len(set(plain_ids[plain_ids >= 0].tolist())) > E.CARS
        _, ids, hits, state = T.track_rows_device(frames, opt, ego=ego)
        assert int(state['next_id']) == E.CARS and sorted(set(ids[ids >= 0].tolist())) == list(range(E.CARS))
        assert T.id_switches(gts, ids) == 0 and hits.max() == len(frames) and np.abs(state['box'][7:10]).max() < 0.1


def device_chunks(frames, ego, opt, cuts):
    """ the sequence in calls of frames[cuts[k]:cuts[k + 1]] with their records, the state carried on the device """
    dev = hip.require_device()
    state = T.state_tensor(None, dev)
    rows, ids, hits = [], [], []
    for a, b in zip(cuts, cuts[1:]):
        r, i, h, state = T.track_rows_device(torch.as_tensor(frames[a:b]).to(dev), opt, state, ego=ego[a:b])
        rows.append(r.cpu().numpy()), ids.append(i.cpu().numpy()), hits.append(h.cpu().numpy())
    return np.concatenate(rows), np.concatenate(ids), np.concatenate(hits), state.cpu().numpy()


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric,thr', E.FOR[1:])
def test_chunked_calls_give_the_same_bytes(metric, thr, assign):
    """ 12 frames in one call, and in 1 + 3 + the rest: the record of a call's first frame relates to the call before """
    frames, ego, _ = E.pitching()
    opt = option(metric, thr, assign, smooth=True, gains=(0.6, 0.3, 0.1))
    whole = device_chunks(frames, ego, opt, [0, 12])
    assert (whole[1] >= 0).sum() == 96 and T.read_state(whole[3])['frames'] == 12 and T.read_state(whole[3])['next_id'] == E.CARS
    for got, want in zip(device_chunks(frames, ego, opt, [0, 1, 4, 12]), whole):
        assert same_bytes(got, want)


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric,thr', E.FOR[1:])
def test_sequences_of_one_call_equal_each_alone(metric, thr, assign):
    """ S = 3 sequences in one launch -- 3 frames of the straight scene, 4 of the curve, 5 of the pitching one --, in front of them a
    frame that belongs to none, whose record is NaN: it is neither checked nor read """
    a, b, c = E.straight(), E.curve(), E.pitching()
    frames = np.concatenate([a[0][:1], a[0][:3], b[0][:4], c[0][:5]])
    ego = np.concatenate([np.full((1, 16), np.nan), a[1][:3], b[1][:4], c[1][:5]])
    seq = [1, 4, 8, 13]
    opt = option(metric, thr, assign, smooth=True)
    rows, ids, hits, states = device_sequences(frames, ego, opt, seq)
    assert states.shape == (3,) and states['frames'].tolist() == [3, 4, 5]
    assert same_bytes(rows[0], frames[0]) and (ids[0] == -1).all() and (hits[0] == 0).all()
    for s, (lo, hi) in enumerate(zip(seq, seq[1:])):
        r, i, h, st = T.track_rows_device(frames[lo:hi], opt, ego=ego[lo:hi])
        assert same_bytes(rows[lo:hi], r) and same_bytes(ids[lo:hi], i) and same_bytes(hits[lo:hi], h) and same_bytes(states[s], st)


def device_sequences(frames, ego, opt, seq):
    """ hip.track itself: utils/track.check_ego would refuse the NaN record of the frame outside every sequence, the entry point must not """
    dev = hip.require_device()
    res = hip.track(torch.as_tensor(frames).to(dev), T.state_tensor(None, dev, len(seq) - 1), T.params_of(opt), seq,
                    optimal=T.is_optimal(opt), ego=ego)
    return res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy(), T.read_state(res[3])


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric,thr', E.FOR[1:])
def test_in_place(metric, thr, assign):
    """ rows_out == rows_in and state_out == state_in """
    frames, ego, _ = E.curve()
    opt = option(metric, thr, assign, smooth=True)
    want = T.track_rows_device(frames, opt, ego=ego)
    dev = hip.require_device()
    rows, state = torch.as_tensor(frames).to(dev), T.state_tensor(None, dev)
    out, ids, hits, state_out = T.track_rows_device(rows, opt, state, out=rows, state_out=state, ego=ego)
    assert out.data_ptr() == rows.data_ptr() and state_out.data_ptr() == state.data_ptr()
    assert same_bytes(rows.cpu().numpy(), want[0]) and same_bytes(ids.cpu().numpy(), want[1]) and same_bytes(hits.cpu().numpy(), want[2])
    assert same_bytes(T.read_state(state)[0], want[3])


@pytest.mark.parametrize('assign', T.ASSIGNS)
def test_one_full_case(assign):
    """ 128 slots against D = 100, one frame, 'dist', a general record: the cars of tests/track_oracle.full_house, then 100 of them seen
    from a camera that has moved and turned.  Equal to the host form (the grid is 8 m wide, the threshold 2.3 m: no margin is near) """
    first = O.full_house()[:1]
    opt = option('dist', None, assign, smooth=True)
    _, _, _, state = T.track_rows_np(first, opt)
    assert int((state['id1'] != 0).sum()) == 128
    pose = E.rot_y(0.04).dot(E.rot_x(0.01))
    pose[:3, 3] = [0.125, -0.03125, -1.5]
    ego = T.ego_records(pose[None])
    rng = np.random.default_rng(5)
    second = first[0][rng.permutation(128)[:100]].astype(np.float64)
    xyz = second[:, [19, 31, 21]].dot(pose[:3, :3].T) + pose[:3, 3] + rng.normal(0.0, 0.05, (100, 3))
    second[:, 19], second[:, 31], second[:, 21], second[:, 32] = xyz[:, 0], xyz[:, 1], xyz[:, 2], ego[0, 12]
    frames = second.astype(np.float32)[None]
    want = T.track_rows_np(frames, opt, state, ego=ego)
    assert (want[2] == 2).sum() == 100 and int(want[3]['next_id']) == 128 and int((want[3]['misses'] == 1).sum()) == 28
    got = T.track_rows_device(frames, opt, state, ego=ego)
    assert same_bytes(got[1], want[1]) and same_bytes(got[2], want[2]) and same_bytes(got[3], want[3]) and rows_agree(got[0], want[0], True)
    assert (T.track_rows_np(frames, opt, state)[2] == 2).sum() < 100              # without the record not every car is found again


def test_nothing_to_do_copies_the_state():
    """ N = 0 and D = 0: GPP_OK, the state is copied """
    frames, ego, _ = E.curve()
    opt = option('dist', 1.0)
    _, _, _, state = T.track_rows_device(frames[:3], opt, ego=ego[:3])
    assert int(state['next_id']) == E.CARS
    for shape in ((0, 3, 36), (2, 0, 36)):
        rows, ids, hits, after = T.track_rows_device(np.zeros(shape, np.float32), opt, state, ego=ego[:shape[0]])
        assert rows.shape == shape and ids.shape == shape[:2] and hits.shape == shape[:2] and same_bytes(after, state)


def test_errors_return_their_code_and_write_nothing():
    """ the new errors of the contract and a short workspace, on live device buffers full of a sentinel """
    dev = hip.require_device()
    frames, ego, _ = E.curve()
    frames, ego = frames[:3], np.ascontiguousarray(ego[:3])
    N, D = frames.shape[:2]
    rows = torch.as_tensor(frames).to(dev)
    nbytes = hip.track_state_bytes()
    sentinel = lambda shape, dtype: torch.full(shape, 77, dtype=dtype, device=dev)  # noqa: E731
    out, ids, hits = sentinel((N, D, 36), torch.float32), sentinel((N, D), torch.int32), sentinel((N, D), torch.int32)
    state_in, state_out = torch.zeros((1, nbytes), dtype=torch.uint8, device=dev), sentinel((1, nbytes), torch.uint8)
    work = torch.zeros((hip.track_ego_workspace_bytes(1, N),), dtype=torch.uint8, device=dev)
    params = hip.TrackParams(metric=2, max_age=2, smooth=0, reserved=0, threshold=1.0, gain_a=0.5, gain_b=0.25, gain_c=0.25, birth_score=0.0)
    seq = (ctypes.c_int32 * 2)(0, N)

    def call(records, assign, work_bytes, p=params):
        e = None if records is None else records.ctypes.data_as(ctypes.c_void_p)
        return hip.lib().gpp_track_ego_f64(hip.ptr(rows), N, D, seq, 1, hip.ptr(state_in), hip.ptr(state_out), ctypes.byref(p), e, assign,
                                           hip.ptr(out), hip.ptr(ids), hip.ptr(hits), hip.ptr(work), work_bytes, hip.stream_ptr())

    def changed(k, value, frame=1):
        bad = ego.copy()
        bad[frame, k] = value
        return bad

    assert call(None, 0, len(work)) == -1
    assert call(ego, 2, len(work)) == -1 and call(ego, -1, len(work)) == -1
    for bad in (changed(0, np.nan), changed(4, np.inf), changed(11, -np.inf), changed(12, np.nan), changed(9, np.nan, 0), changed(2, np.inf, 2),
                changed(13, 1.0), changed(14, -0.5), changed(15, np.nan)):
        assert call(bad, 0, len(work)) == -1 and call(bad, 1, len(work)) == -1
    assert call(ego, 0, len(work) - 8) == -2 and call(ego, 1, hip.track_workspace_bytes(1)) == -2      # the plain size is short
    bad_params = hip.TrackParams(metric=2, max_age=2, smooth=0, reserved=1, threshold=1.0, gain_a=0.5, gain_b=0.25, gain_c=0.25, birth_score=0.0)
    assert call(ego, 0, len(work), bad_params) == -1                                                   # (an error of gpp_track_f64's)
    torch.cuda.synchronize()
    for t in (out, ids, hits, state_out):
        assert bool((t == 77).all())
    # the same buffers, a good call: it does write
    assert call(ego, 0, len(work)) == 0
    want = T.track_rows_np(frames, O.options('dist', 1.0), ego=ego)
    assert same_bytes(ids.cpu().numpy(), want[1]) and same_bytes(out.cpu().numpy(), frames) and same_bytes(T.read_state(state_out)[0], want[3])


# ---------------------------------------------------------------------------------------------------- the model
def noise_frames(n, h, w, seed):
    """ binary noise: keeps the synthetic weights' scores above the 0.05 threshold """
    return (np.random.default_rng(seed).integers(0, 2, size=(n, h, w, 3)) * 255).astype(np.uint8)


def calibration(B, n_planes='100'):
    planes = synthetic.load_plane_database(n_planes).astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))


def model_against_the_host_form(weights, opt, f, P_inv, planes, ego):
    """ 2 + 2 frames through predict_tracks_on_frames against track_rows_np over the rows predict_poses_on_frames gives for the same
    frames, with the same records (None: a model without 'ego') """
    model = models.load_model(weights, backbone_name='resnet50', dtype='f32', pose=True, track=opt)
    more = (lambda a, b: {}) if ego is None else (lambda a, b: {'ego': ego[a:b]})
    (rows_a, _, ids_a, hits_a), _ = model.predict_tracks_on_frames(f[:2], P_inv, planes, **more(0, 2))
    (pose_a, _), _ = model.predict_poses_on_frames(f[:2], P_inv, planes)
    (pose_b, _), _ = model.predict_poses_on_frames(f[2:], P_inv, planes)
    (rows_b, _, ids_b, hits_b), _ = model.predict_tracks_on_frames(f[2:], P_inv, planes, **more(2, 4))
    state = model.track_state()
    pose = np.concatenate([pose_a, pose_b])
    assert pose.shape == (4, 100, 36) and (pose[:, :, 14] >= 0).sum() >= 4                  # there is something to track
    want_rows, want_ids, want_hits, want_state = T.track_rows_np(pose, opt, ego=ego)
    ids, hits, rows = np.concatenate([ids_a, ids_b]), np.concatenate([hits_a, hits_b]), np.concatenate([rows_a, rows_b])
    assert same_bytes(ids, want_ids) and same_bytes(hits, want_hits)
    assert same_bytes(state, want_state) and int(state['frames']) == 4 and int(state['next_id']) > 0
    assert rows_agree(rows, want_rows, True)
    return model, pose, state


def test_model_tracks_with_records_equal_the_host_form_and_a_plain_model_after_it_is_unchanged(monkeypatch):
    """ the model launches the entry point its option names: 'ego': True equals the host form with the same records over the model's own
    pose rows (and not the host form without them: the records did reach the kernel); the missing and the superfluous `ego` are refused
    before anything is staged; then, with the same weights, a model without 'ego' still equals the plain host form """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    weights = W.synthetic_weights('resnet50', 1234)
    f = noise_frames(4, 96, 160, seed=5)
    P_inv, planes = calibration(2)
    opt = {'metric': 'dist', 'threshold': 2.0, 'smooth': True}
    ego = E.curve()[1][:4]
    model, pose, state = model_against_the_host_form(weights, dict(opt, ego=True), f, P_inv, planes, ego)
    assert model.track['ego'] is True and model._track_ego_work[0] == 2
    assert not same_bytes(state, T.track_rows_np(pose, opt)[3])
    with pytest.raises(hip.GppError, match='needs ego=records'):
        model.predict_tracks_on_frames(f[:2], P_inv, planes)
    with pytest.raises(hip.GppError, match='one record per frame'):
        model.predict_tracks_on_frames(f[:2], P_inv, planes, ego=ego[:3])
    assert same_bytes(model.track_state(), state)                                           # a refusal stages and advances nothing
    plain, _, _ = model_against_the_host_form(weights, opt, f, P_inv, planes, None)
    assert 'ego' not in plain.track and plain._track_ego_work is None
    with pytest.raises(hip.GppError, match="not loaded with track="):
        plain.predict_tracks_on_frames(f[:2], P_inv, planes, ego=ego[:2])
