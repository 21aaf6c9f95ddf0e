""" GPU tests of the tracker (csrc/track.hip): the kernel against the NumPy form (utils/track.py) and the
loop-written oracle (tests/track_oracle.py) on the cases of tests/test_track_cpu.py, which asserts their margins; chunked calls, several
sequences in one call, in place; the contract's errors; RetinaNet3D(pose=True, track=...) end to end; the two command lines. """
import ctypes

import numpy as np
import pytest
import torch

import track_oracle as O
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import synthetic
from keras_retinanet_3D.utils import track as T

pytestmark = pytest.mark.gpu

EXACT = O.exact_cases()
MARGIN = O.margin_cases()
MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def alpha_within_4_ulp(got, want):
    """ column 25 of smoothed rows: 4 float32 ulp of the oracle's value (the bar of tests/test_pose_gpu.py); bit-equal elsewhere """
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    return bool((same | (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 4 * np.spacing(np.abs(want)).astype(np.float64))).all())


def rows_agree(got, want, smooth):
    cols = [c for c in range(36) if c != 25 or not smooth]
    return same_bytes(got[..., cols], want[..., cols]) and alpha_within_4_ulp(got[..., 25], want[..., 25])


@pytest.mark.parametrize('name,frames,opt', EXACT + MARGIN, ids=[c[0] for c in EXACT + MARGIN])
def test_kernel_equals_the_host_form_and_the_oracle(name, frames, opt):
    """ ids, hits and every state field: ==.  r_y = 0 with dyadic numbers, or the margins that tests/test_track_cpu.py asserts """
    o_rows, o_ids, o_hits, o_state = O.track(frames, opt)
    n_rows, n_ids, n_hits, n_state = T.track_rows_np(frames, opt)
    rows, ids, hits, state = T.track_rows_device(frames, opt)
    assert rows.dtype == np.float32 and ids.dtype == np.int32 and hits.dtype == np.int32 and rows.shape == frames.shape
    assert np.array_equal(ids, n_ids) and np.array_equal(ids, o_ids)
    assert np.array_equal(hits, n_hits) and np.array_equal(hits, o_hits)
    assert same_bytes(state, n_state) and O.same_state(o_state, state)
    assert rows_agree(rows, o_rows, opt['smooth']) and rows_agree(rows, n_rows, opt['smooth'])
    if not opt['smooth']:
        assert same_bytes(rows, frames)


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
    """ case 7: 12 frames in one call, in 5 + 7, in twelve calls of one """
    frames = O.drive(O.DRIVE_SEED)
    opt = O.options(metric, smooth=True, gains=(0.6, 0.3, 0.1))
    whole = device_chunks(frames, opt, [0, 12])
    assert (whole[1] >= 0).sum() > 40 and T.read_state(whole[3])['frames'] == 12
    for cuts in ([0, 5, 12], list(range(13))):
        for got, want in zip(device_chunks(frames, opt, cuts), whole):
            assert same_bytes(got, want)


@pytest.mark.parametrize('metric', T.METRICS)
def test_sequences_of_one_call_equal_each_alone(metric):
    """ case 8: S = 3 sequences of 1, 4 and 7 frames, in front of them a frame that belongs to none """
    frames = np.concatenate([O.drive(3, frames=1), O.drive(O.DRIVE_SEED)])
    seq = [1, 2, 6, 13]
    opt = O.options(metric, smooth=True)
    rows, ids, hits, states = T.track_rows_device(frames, opt, seq_start=seq)
    assert states.shape == (3,) and states['frames'].tolist() == [1, 4, 7]
    assert same_bytes(rows[0], frames[0]) and (ids[0] == -1).all() and (hits[0] == 0).all()
    for s, (a, b) in enumerate(zip(seq, seq[1:])):
        r, i, h, st = T.track_rows_device(frames[a:b], opt)
        assert same_bytes(rows[a:b], r) and same_bytes(ids[a:b], i) and same_bytes(hits[a:b], h) and same_bytes(states[s], st)
    # ... and with states that differ on entry
    entry = np.stack([states[2], T.empty_state(), states[0]])
    rows2, ids2, _, states2 = T.track_rows_device(frames, opt, state=entry, seq_start=seq)
    r, i, _, st = T.track_rows_device(frames[1:2], opt, state=states[2])
    assert same_bytes(rows2[1:2], r) and same_bytes(ids2[1:2], i) and same_bytes(states2[0], st) and same_bytes(ids2[2:6], ids[2:6])


@pytest.mark.parametrize('metric', T.METRICS)
def test_in_place(metric):
    """ case 9: rows_out == rows_in and state_out == state_in """
    frames = O.drive(O.DRIVE_SEED)
    opt = O.options(metric, smooth=True)
    want = T.track_rows_device(frames, opt)
    dev = hip.require_device()
    rows, state = torch.as_tensor(frames).to(dev), T.state_tensor(None, dev)
    out, ids, hits, state_out = T.track_rows_device(rows, opt, state, out=rows, state_out=state)
    assert out.data_ptr() == rows.data_ptr() and state_out.data_ptr() == state.data_ptr()
    assert same_bytes(rows.cpu().numpy(), want[0]) and same_bytes(ids.cpu().numpy(), want[1]) and same_bytes(hits.cpu().numpy(), want[2])
    assert same_bytes(T.read_state(state)[0], want[3])


def test_nothing_to_do_copies_the_state():
    """ case 5's N = 0 and D = 0: GPP_OK, the state is copied """
    frames = O.crossing()
    _, _, _, state = T.track_rows_device(frames[:3], ('dist', O.DIST_THR))
    assert int(state['next_id']) == 2
    for shape in ((0, 3, 36), (2, 0, 36)):
        rows, ids, hits, after = T.track_rows_device(np.zeros(shape, np.float32), ('dist', O.DIST_THR), state)
        assert rows.shape == shape and ids.shape == shape[:2] and hits.shape == shape[:2] and same_bytes(after, state)


def test_errors_return_their_code_and_write_nothing():
    """ case 10: every error of the contract, on live device buffers full of a sentinel """
    dev = hip.require_device()
    frames = O.crossing()[:4]
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
               dict(max_age=-1), dict(birth_score=nan)]
    calls = [(hip.TrackParams(**dict(good, **c)), [0, N], False, len(work), -1) for c in changes]
    calls += [(hip.TrackParams(**good), [2, 1], False, len(work), -1), (hip.TrackParams(**good), [0, N + 1], False, len(work), -1),
              (hip.TrackParams(**good), [0, N], True, len(work), -4), (hip.TrackParams(**good), [0, N], False, len(work) - 8, -2)]
    for params, seq, big, work_bytes, code in calls:
        seq = (ctypes.c_int32 * 2)(*seq)
        r, o, i, h = (big_rows, big_out, big_ids, big_hits) if big else (rows, out, ids, hits)
        rc = hip.lib().gpp_track_f64(hip.ptr(r), N, int(r.shape[1]), seq, 1, hip.ptr(state_in), hip.ptr(state_out), ctypes.byref(params),
                                     hip.ptr(o), hip.ptr(i), hip.ptr(h), hip.ptr(work), work_bytes, hip.stream_ptr())
        assert rc == code, (rc, code)
    torch.cuda.synchronize()
    for t in (out, ids, hits, big_out, big_ids, big_hits, state_out):
        assert bool((t == 77).all())
    # the same buffers, a good call: it does write
    seq = (ctypes.c_int32 * 2)(0, N)
    params = hip.TrackParams(**good)
    assert hip.lib().gpp_track_f64(hip.ptr(rows), N, D, seq, 1, hip.ptr(state_in), hip.ptr(state_out), ctypes.byref(params), hip.ptr(out),
                                   hip.ptr(ids), hip.ptr(hits), hip.ptr(work), len(work), hip.stream_ptr()) == 0
    assert same_bytes(ids.cpu().numpy(), T.track_rows_np(frames, ('dist', 2.0))[1]) and same_bytes(out.cpu().numpy(), frames)


# ---------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope='module')
def weights50():
    return W.synthetic_weights('resnet50', 1234)


def noise_frames(n, h, w, seed):
    """ binary noise: keeps the synthetic weights' scores above the 0.05 threshold """
    return (np.random.default_rng(seed).integers(0, 2, size=(n, h, w, 3)) * 255).astype(np.uint8)


def calibration(B, n_planes='100'):
    planes = synthetic.load_plane_database(n_planes).astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))


def test_model_tracks_equal_the_host_form_over_its_pose_rows(weights50, monkeypatch):
    """ 2 + 2 frames through predict_tracks_on_frames against track_rows_np over the rows predict_poses_on_frames gives for the same four
    frames -- called between the two track calls, which it must not disturb; then reset_tracks brings back id 0 """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    option = {'metric': 'dist', 'threshold': 6.0, 'max_age': 1, 'smooth': True}
    model = models.load_model(weights50, backbone_name='resnet50', dtype='f32', pose=True, track=option)
    f = noise_frames(4, 96, 160, seed=5)
    P_inv, planes = calibration(2)
    assert int(model.track_state()['frames']) == 0
    (rows_a, counts_a, ids_a, hits_a), scale = model.predict_tracks_on_frames(f[:2], P_inv, planes)
    (pose_a, pcounts_a), _ = model.predict_poses_on_frames(f[:2], P_inv, planes)
    (pose_b, pcounts_b), _ = model.predict_poses_on_frames(f[2:], P_inv, planes)
    assert int(model.track_state()['frames']) == 2
    (rows_b, counts_b, ids_b, hits_b), _ = model.predict_tracks_on_frames(f[2:], P_inv, planes)
    state = model.track_state()
    pose = np.concatenate([pose_a, pose_b])
    assert pose.shape == (4, 100, 36) and (pose[:, :, 14] >= 0).sum() >= 4                  # there is something to track
    want_rows, want_ids, want_hits, want_state = T.track_rows_np(pose, option)
    ids, hits, rows = np.concatenate([ids_a, ids_b]), np.concatenate([hits_a, hits_b]), np.concatenate([rows_a, rows_b])
    assert ids.dtype == np.int32 and ids.shape == (4, 100) and same_bytes(ids, want_ids) and same_bytes(hits, want_hits)
    assert same_bytes(state, want_state) and int(state['frames']) == 4 and int(state['next_id']) > 0
    assert rows_agree(rows, want_rows, True) and not same_bytes(rows, pose)                 # smoothed: the filter's cuboids
    assert same_bytes(np.concatenate([counts_a, counts_b]), np.concatenate([pcounts_a, pcounts_b]))
    assert ((ids >= 0) == (pose[:, :, 14] >= 0)).all()                                       # birth_score 0: every detection has an id
    model.reset_tracks()
    (_, _, ids_c, hits_c), _ = model.predict_tracks_on_frames(f[:2], P_inv, planes)
    assert same_bytes(ids_c, ids_a) and same_bytes(hits_c, hits_a) and ids_c.min() == -1 and 0 in ids_c[0]
    assert int(model.track_state()['frames']) == 2
    plain = models.load_model(weights50, backbone_name='resnet50', dtype='f32', pose=True)
    with pytest.raises(hip.GppError):
        plain.predict_tracks_on_frames(f[:2], P_inv, planes)
    with pytest.raises(hip.GppError):
        plain.track_state()


def test_range_event_advances_the_state_once_by_the_twins_rows(weights50, monkeypatch):
    """ the weights of tests/test_pose_gpu.py's test_range_event_answers_with_the_twins_rows: the float32 twin answers the call; the
    reader has then run twice, and the state has advanced once, by the twin's rows """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    B, h, w = 2, 96, 160
    scaled = dict(weights50)
    k = np.float32(2.0 ** 17)
    scaled['bn2a_branch2a/gamma'], scaled['bn2a_branch2a/beta'] = scaled['bn2a_branch2a/gamma'] * k, scaled['bn2a_branch2a/beta'] * k
    scaled['res2a_branch2b/kernel'] = scaled['res2a_branch2b/kernel'] / k
    option = ('dist', 6.0)
    tracked = models.load_model(scaled, backbone_name='resnet50', dtype='f16x3', pose=True, track=option)
    m32 = models.load_model(scaled, backbone_name='resnet50', dtype='f32', pose=True)
    P_inv, planes = calibration(B)
    x = np.random.default_rng(0).integers(0, 256, size=(B, h, w, 3)).astype(np.float32) - MEAN
    inputs = [x, P_inv, planes]
    rows, counts, ids, hits = tracked.predict_tracks_on_batch(inputs, 1.25, (h, w, 3))
    assert tracked.range_fallbacks == 1
    want_rows, want_counts = m32.predict_poses_on_batch(inputs, 1.25, (h, w, 3))
    assert same_bytes(rows, want_rows) and same_bytes(counts, want_counts)
    _, want_ids, want_hits, want_state = T.track_rows_np(want_rows, option)
    state = tracked.track_state()
    assert int(state['frames']) == B and same_bytes(state, want_state) and same_bytes(ids, want_ids) and same_bytes(hits, want_hits)
    # the next call continues from there
    rows2, _, ids2, hits2 = tracked.predict_tracks_on_batch(inputs, 1.25, (h, w, 3))
    _, want_ids2, want_hits2, want_state2 = T.track_rows_np(want_rows, option, want_state)
    assert tracked.range_fallbacks == 2 and same_bytes(ids2, want_ids2) and same_bytes(hits2, want_hits2)
    assert same_bytes(tracked.track_state(), want_state2) and int(want_state2['frames']) == 2 * B


def test_command_lines_write_the_host_forms_tracks(weights50, tmp_path, monkeypatch):
    """ bin/run_network.py --track against tracking_lines over track_rows_np of the rows its calls returned; bin/track_results.py on the
    result files it wrote, on the device and with --host """
    from PIL import Image
    from keras_retinanet_3D.bin import run_network, track_results
    from keras_retinanet_3D.models import retinanet
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    (tmp_path / 'img').mkdir(); (tmp_path / 'calib').mkdir(); (tmp_path / 'out').mkdir()
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    for k in range(3):
        Image.fromarray(noise_frames(1, 375, 1242, k)[0][:, :, ::-1]).save(str(tmp_path / 'img' / ('%06d.png' % k)))
        (tmp_path / 'calib' / ('%06d.txt' % k)).write_text(calib)
    seen = []
    inner = retinanet.RetinaNet3D.predict_tracks_on_frames

    def recording(self, *args):
        result = inner(self, *args)
        seen.append(result[0])
        return result
    monkeypatch.setattr(retinanet.RetinaNet3D, 'predict_tracks_on_frames', recording)
    run_network.main(['synthetic:1234.h5', str(tmp_path / 'img'), str(tmp_path / 'calib'), synthetic.plane_database_path('1k'), str(tmp_path / 'out'),
                      '--kitti', '--batch-size', '2', '--device-pose', '--track', 'dist', '--track-threshold', '8', '--track-max-age', '1'])
    assert [s[0].shape[0] for s in seen] == [2, 1]
    rows = np.concatenate([s[0] for s in seen])
    option = {'metric': 'dist', 'threshold': 8.0, 'max_age': 1}
    _, ids, hits, _ = T.track_rows_np(rows, option)
    assert same_bytes(ids, np.concatenate([s[2] for s in seen])) and (ids >= 0).sum() >= 3
    want = ''.join(T.tracking_lines(k, rows[k], ids[k], hits[k]) for k in range(3))
    root = tmp_path / 'out' / 'synthetic:1234' / 'outputs'
    text = (root / 'tracking' / 'tracks.txt').read_text()
    assert text == want and text.count('\n') == int((ids >= 0).sum())
    assert [int(line.split()[0]) for line in text.splitlines()] == sorted(int(line.split()[0]) for line in text.splitlines())
    # the result files, tracked again without the network
    common = [str(root / 'kitti'), '--metric', 'dist', '--threshold', '8', '--max-age', '1', '--min-hits', '2']
    track_results.main([common[0], str(tmp_path / 'device.txt')] + common[1:])
    track_results.main([common[0], str(tmp_path / 'host.txt')] + common[1:] + ['--host'])
    names, frames = track_results.read_sequence(str(root / 'kitti'))
    _, ids, hits, _ = T.track_rows_np(frames, option)
    want = ''.join(T.tracking_lines(k, frames[k], ids[k], hits[k], 2) for k in range(3))
    assert names == ['%06d.txt' % k for k in range(3)]
    assert (tmp_path / 'device.txt').read_text() == want and (tmp_path / 'host.txt').read_text() == want
