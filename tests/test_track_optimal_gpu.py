""" GPU tests of the tracker's optimal assignment (csrc/track.hip, gpp_track_optimal_f64): the kernel against the
NumPy form (utils/track.py) and the loop-written oracle (tests/track_optimal_oracle.py) on the cases of tests/test_track_optimal_cpu.py,
which asserts their margins; chunked calls, several sequences in one call, in place; the contract's errors; RetinaNet3D(pose=True,
track={..., 'assign': 'optimal'}) end to end, and a greedy model after it. """
import ctypes

import numpy as np
import pytest
import torch

import track_optimal_oracle as P
import track_oracle as O
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import synthetic
from keras_retinanet_3D.utils import track as T

pytestmark = pytest.mark.gpu

EXACT = P.exact_cases()
MARGIN = P.margin_cases()


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


@pytest.mark.parametrize('name,frames,opt', EXACT + MARGIN, ids=[c[0] for c in EXACT + MARGIN])
def test_kernel_equals_the_host_form_and_the_oracle(name, frames, opt):
    """ ids, hits and every state field: ==.  r_y = 0 with dyadic numbers, or the margins that tests/test_track_optimal_cpu.py asserts """
    assert opt['assign'] == 'optimal'
    o_rows, o_ids, o_hits, o_state = P.track(frames, opt)
    n_rows, n_ids, n_hits, n_state = T.track_rows_np(frames, opt)
    rows, ids, hits, state = T.track_rows_device(frames, opt)
    assert rows.dtype == np.float32 and ids.dtype == np.int32 and hits.dtype == np.int32 and rows.shape == frames.shape
    assert np.array_equal(ids, n_ids) and np.array_equal(ids, o_ids)
    assert np.array_equal(hits, n_hits) and np.array_equal(hits, o_hits)
    assert same_bytes(state, n_state) and O.same_state(o_state, state)
    assert rows_agree(rows, o_rows, opt['smooth']) and rows_agree(rows, n_rows, opt['smooth'])
    if not opt['smooth']:
        assert same_bytes(rows, frames)


def test_the_cases_reach_the_branches_they_name():
    """ the shapes of the new exact cases, on the device's results: the steal, the second column of a lane, the full matrix """
    case = {c[0]: c for c in EXACT}
    run = lambda name: T.track_rows_device(*case[name][1:])  # noqa: E731
    assert run('steal_dist')[1].tolist() == [[0, 1], [1, 0]]
    assert T.track_rows_device(P.steal(), P.STEAL_OPTION)[1].tolist() == [[0, 1], [0, 2]]              # the greedy entry point, the same rows
    for metric in T.METRICS:
        assert run('one_slot_three_rows_' + metric)[1].tolist() == [[0, -1, -1], [1, 0, 2]]          # the nearest row continues the track
        _, ids, _, state = run('three_slots_one_row_' + metric)
        assert ids.tolist() == [[0, 1, 2], [1, -1, -1]] and state['misses'][:3].tolist() == [1, 0, 1]
        assert run('one_sided_' + metric)[1].tolist() == [[-1, -1], [0, -1], [-1, -1], [0, -1]]
        _, ids, hits, state = run('many_slots_two_rows_' + metric)
        assert ids[1, :2].tolist() == [64, 3] and hits[1, :2].tolist() == [2, 2] and int((state['misses'] == 1).sum()) == 63
        _, ids, hits, state = run('two_slots_many_rows_' + metric)
        assert ids[1, 64] == 0 and ids[1, 3] == 1 and hits[1, [64, 3]].tolist() == [2, 2] and int(state['next_id']) == 65
        assert run('tie_rows_' + metric)[1].tolist() == [[0, -1], [0, 1]]                             # the first column
        assert run('tie_slots_' + metric)[1].tolist() == [[0, 1], [0, -1]]                            # the first row
    for metric in ('dist', 'bev'):
        _, ids, _, state = run('full_house_' + metric)
        assert ids[0].tolist() == list(range(128)) and ids[1].tolist() == list(range(127)) + [-1] and int(state['dropped']) == 1


def test_every_pair_a_candidate_at_equal_cells():
    """ 128 slots against 128 rows with every cell equal (the most dependent steps the rule allows): row j keeps slot j """
    car = P.row(0.9, 0.5, 20.0)
    frames = np.stack([np.stack([car] * 128)] * 2)
    opt = P.optimal(O.options('dist', threshold=2.0))
    rows, ids, hits, state = T.track_rows_device(frames, opt)
    n_rows, n_ids, n_hits, n_state = T.track_rows_np(frames, opt)
    assert ids[1].tolist() == list(range(128)) and (hits[1] == 2).all()
    assert same_bytes(ids, n_ids) and same_bytes(hits, n_hits) and same_bytes(state, n_state) and same_bytes(rows, frames)


def device_chunks(frames, opt, cuts):
    """ the sequence in calls of frames[cuts[k]:cuts[k + 1]], the state carried on the device """
    dev = hip.require_device()
    state = T.state_tensor(None, dev)
    rows, ids, hits = [], [], []
    for a, b in zip(cuts, cuts[1:]):
        r, i, h, state = T.track_rows_device(torch.as_tensor(frames[a:b]).to(dev), opt, state)
        rows.append(r.cpu().numpy()), ids.append(i.cpu().numpy()), hits.append(h.cpu().numpy())
    return np.concatenate(rows), np.concatenate(ids), np.concatenate(hits), state.cpu().numpy()


@pytest.mark.parametrize('metric', T.METRICS)
def test_chunked_calls_give_the_same_bytes(metric):
    """ 12 frames in one call, and in 1 + 3 + the rest """
    frames = O.drive(O.DRIVE_SEED)
    opt = P.optimal(O.options(metric, smooth=True, gains=(0.6, 0.3, 0.1)))
    whole = device_chunks(frames, opt, [0, 12])
    assert (whole[1] >= 0).sum() > 40 and T.read_state(whole[3])['frames'] == 12
    for got, want in zip(device_chunks(frames, opt, [0, 1, 4, 12]), whole):
        assert same_bytes(got, want)


@pytest.mark.parametrize('metric', T.METRICS)
def test_sequences_of_one_call_equal_each_alone(metric):
    """ S = 3 sequences of different n in one launch -- 2 frames of the dense drive (D = 16), 4 and 7 of the drive --, in front of them
    a frame that belongs to none """
    frames = np.concatenate([O.drive(3, frames=1), P.dense_drive()[:2], O.drive(O.DRIVE_SEED)[:11]])
    seq = [1, 3, 7, 14]
    opt = P.optimal(O.options(metric, smooth=True))
    rows, ids, hits, states = T.track_rows_device(frames, opt, seq_start=seq)
    assert states.shape == (3,) and states['frames'].tolist() == [2, 4, 7]
    assert same_bytes(rows[0], frames[0]) and (ids[0] == -1).all() and (hits[0] == 0).all()
    for s, (a, b) in enumerate(zip(seq, seq[1:])):
        r, i, h, st = T.track_rows_device(frames[a:b], opt)
        assert same_bytes(rows[a:b], r) and same_bytes(ids[a:b], i) and same_bytes(hits[a:b], h) and same_bytes(states[s], st)
    # ... and with states that differ on entry
    entry = np.stack([states[2], T.empty_state(), states[0]])
    rows2, ids2, _, states2 = T.track_rows_device(frames, opt, state=entry, seq_start=seq)
    r, i, _, st = T.track_rows_device(frames[1:3], opt, state=states[2])
    assert same_bytes(rows2[1:3], r) and same_bytes(ids2[1:3], i) and same_bytes(states2[0], st) and same_bytes(ids2[3:7], ids[3:7])


@pytest.mark.parametrize('metric', T.METRICS)
def test_in_place(metric):
    """ rows_out == rows_in and state_out == state_in """
    frames = O.drive(O.DRIVE_SEED)
    opt = P.optimal(O.options(metric, smooth=True))
    want = T.track_rows_device(frames, opt)
    dev = hip.require_device()
    rows, state = torch.as_tensor(frames).to(dev), T.state_tensor(None, dev)
    out, ids, hits, state_out = T.track_rows_device(rows, opt, state, out=rows, state_out=state)
    assert out.data_ptr() == rows.data_ptr() and state_out.data_ptr() == state.data_ptr()
    assert same_bytes(rows.cpu().numpy(), want[0]) and same_bytes(ids.cpu().numpy(), want[1]) and same_bytes(hits.cpu().numpy(), want[2])
    assert same_bytes(T.read_state(state)[0], want[3])


def test_nothing_to_do_copies_the_state():
    """ N = 0 and D = 0: GPP_OK, the state is copied """
    option = P.optimal(O.options('dist'))
    _, _, _, state = T.track_rows_device(O.crossing()[:3], option)
    assert int(state['next_id']) == 2
    for shape in ((0, 3, 36), (2, 0, 36)):
        rows, ids, hits, after = T.track_rows_device(np.zeros(shape, np.float32), option, state)
        assert rows.shape == shape and ids.shape == shape[:2] and hits.shape == shape[:2] and same_bytes(after, state)


def test_errors_return_their_code_and_write_nothing():
    """ every error of the contract, on live device buffers full of a sentinel """
    dev = hip.require_device()
    frames = P.steal()
    N, D = frames.shape[:2]
    rows = torch.as_tensor(frames).to(dev)
    nbytes = hip.track_state_bytes()
    sentinel = lambda shape, dtype: torch.full(shape, 77, dtype=dtype, device=dev)  # noqa: E731
    out, ids, hits = sentinel((N, D, 36), torch.float32), sentinel((N, D), torch.int32), sentinel((N, D), torch.int32)
    big_rows, big_out = torch.zeros((N, 129, 36), dtype=torch.float32, device=dev), sentinel((N, 129, 36), torch.float32)
    big_ids, big_hits = sentinel((N, 129), torch.int32), sentinel((N, 129), torch.int32)
    state_in, state_out = torch.zeros((1, nbytes), dtype=torch.uint8, device=dev), sentinel((1, nbytes), torch.uint8)
    work = torch.zeros((hip.track_workspace_bytes(1),), dtype=torch.uint8, device=dev)
    good = dict(metric=2, max_age=2, smooth=0, reserved=0, threshold=2.0, gain_a=0.5, gain_b=0.25, gain_c=0.25, birth_score=0.0)
    nan = float('nan')
    changes = [dict(metric=3), dict(metric=0, threshold=1.0), dict(metric=1, threshold=-0.5), dict(metric=0, threshold=nan),
               dict(threshold=0.0), dict(threshold=float('inf')), dict(threshold=nan), dict(gain_a=0.0), dict(gain_a=1.5), dict(gain_a=nan),
               dict(gain_b=-0.5), dict(gain_b=1.5), dict(gain_b=nan), dict(gain_c=-0.5), dict(gain_c=1.5), dict(gain_c=nan),
               dict(max_age=-1), dict(birth_score=nan), dict(smooth=2), dict(reserved=1)]
    calls = [(hip.TrackParams(**dict(good, **c)), [0, N], False, len(work), -1) for c in changes]
    calls += [(hip.TrackParams(**good), [2, 1], False, len(work), -1), (hip.TrackParams(**good), [0, N + 1], False, len(work), -1),
              (hip.TrackParams(**good), [0, N], True, len(work), -4), (hip.TrackParams(**good), [0, N], False, len(work) - 8, -2)]
    for params, seq, big, work_bytes, code in calls:
        seq = (ctypes.c_int32 * 2)(*seq)
        r, o, i, h = (big_rows, big_out, big_ids, big_hits) if big else (rows, out, ids, hits)
        rc = hip.lib().gpp_track_optimal_f64(hip.ptr(r), N, int(r.shape[1]), seq, 1, hip.ptr(state_in), hip.ptr(state_out), ctypes.byref(params),
                                             hip.ptr(o), hip.ptr(i), hip.ptr(h), hip.ptr(work), work_bytes, hip.stream_ptr())
        assert rc == code, (rc, code)
    torch.cuda.synchronize()
    for t in (out, ids, hits, big_out, big_ids, big_hits, state_out):
        assert bool((t == 77).all())
    # the same buffers, a good call: it does write
    seq = (ctypes.c_int32 * 2)(0, N)
    params = hip.TrackParams(**good)
    assert hip.lib().gpp_track_optimal_f64(hip.ptr(rows), N, D, seq, 1, hip.ptr(state_in), hip.ptr(state_out), ctypes.byref(params), hip.ptr(out),
                                           hip.ptr(ids), hip.ptr(hits), hip.ptr(work), len(work), hip.stream_ptr()) == 0
    assert ids.cpu().numpy().tolist() == [[0, 1], [1, 0]] and same_bytes(out.cpu().numpy(), frames)


# ---------------------------------------------------------------------------------------------------- the model
def noise_frames(n, h, w, seed):
    """ binary noise: keeps the synthetic weights' scores above the 0.05 threshold """
    return (np.random.default_rng(seed).integers(0, 2, size=(n, h, w, 3)) * 255).astype(np.uint8)


def calibration(B, n_planes='100'):
    planes = synthetic.load_plane_database(n_planes).astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))


def model_against_the_host_form(weights, option, f, P_inv, planes):
    """ 2 + 2 frames through predict_tracks_on_frames against track_rows_np over the rows predict_poses_on_frames gives for the same
    frames """
    model = models.load_model(weights, backbone_name='resnet50', dtype='f32', pose=True, track=option)
    (rows_a, _, ids_a, hits_a), _ = model.predict_tracks_on_frames(f[:2], P_inv, planes)
    (pose_a, _), _ = model.predict_poses_on_frames(f[:2], P_inv, planes)
    (pose_b, _), _ = model.predict_poses_on_frames(f[2:], P_inv, planes)
    (rows_b, _, ids_b, hits_b), _ = model.predict_tracks_on_frames(f[2:], P_inv, planes)
    state = model.track_state()
    pose = np.concatenate([pose_a, pose_b])
    assert pose.shape == (4, 100, 36) and (pose[:, :, 14] >= 0).sum() >= 4                  # there is something to track
    want_rows, want_ids, want_hits, want_state = T.track_rows_np(pose, option)
    ids, hits, rows = np.concatenate([ids_a, ids_b]), np.concatenate([hits_a, hits_b]), np.concatenate([rows_a, rows_b])
    assert same_bytes(ids, want_ids) and same_bytes(hits, want_hits) and (hits > 1).any()    # tracks do continue
    assert same_bytes(state, want_state) and int(state['frames']) == 4 and int(state['next_id']) > 0
    assert rows_agree(rows, want_rows, True) and not same_bytes(rows, pose)                 # smoothed: the filter's cuboids
    return model


def test_model_tracks_equal_the_host_form_and_a_greedy_model_after_it_is_unchanged(monkeypatch):
    """ the model launches the entry point its option names: 'assign': 'optimal' equals the optimal host form over the model's own pose
    rows; then, with the same weights, a greedy model still equals the greedy host form """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    weights = W.synthetic_weights('resnet50', 1234)
    f = noise_frames(4, 96, 160, seed=5)
    P_inv, planes = calibration(2)
    option = {'metric': 'dist', 'threshold': 6.0, 'max_age': 1, 'smooth': True}
    best = model_against_the_host_form(weights, dict(option, assign='optimal'), f, P_inv, planes)
    assert best.track['assign'] == 'optimal' and best._track_optimal
    greedy = model_against_the_host_form(weights, option, f, P_inv, planes)
    assert 'assign' not in greedy.track and not greedy._track_optimal
