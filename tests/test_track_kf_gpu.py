""" GPU tests of the tracker's Kalman filter (csrc/track.hip, gpp_track_kf_f64): the kernel against the NumPy form
(utils/track.py) and the loop-written oracle (tests/track_kf_oracle.py) on the cases of tests/test_track_kf_cpu.py, which asserts their
margins -- (greedy or optimal) x (records or none) x ('maha' or 'dist' with the filter), and 'bev' once --; the demonstration scene;
chunked calls; in place; nothing to do; a caller's covariance that takes the fallback; one crowded frame of 128 slots x 128 rows
through optimal + ego + Kalman and through greedy + Kalman; RetinaNet3D(pose=True, track={..., 'filter': 'kalman'}) end to end, and a
range event that advances state and covariance once.

'maha' and 'dist' decide on + - * / and sqrt alone, which are correctly rounded on both sides: the equality there is unconditional.
Under 'bev' cos / sin take part in the overlaps, and the CPU-asserted 1e-9 margins keep their last bit out of every decision. """
import ctypes

import numpy as np
import pytest
import torch

import test_track_kf_cpu as H
import track_kf_oracle as K
import track_oracle as O
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import synthetic
from keras_retinanet_3D.utils import track as T

pytestmark = pytest.mark.gpu

MEAN = np.array([103.939, 116.779, 123.68], np.float32)
# every case of 'maha' and of 'dist' with the filter -- both assignments, no records / identity / quarter turns / one general rotation --,
# and 'bev' once per assignment, on the drive without records
CASES = [c for c in K.cases() if '_maha_' in c[0] or '_dist_' in c[0] or c[0] in ('drive_bev_greedy', 'drive_bev_optimal')]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def alpha_within_4_ulp(got, want):
    """ column 25 of smoothed rows: 4 float32 ulp of the other form's value (the bar of tests/test_track_gpu.py); bit-equal elsewhere """
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    return bool((same | (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 4 * np.spacing(np.abs(want)).astype(np.float64))).all())


def rows_agree(got, want, smooth):
    cols = [c for c in range(36) if c != 25 or not smooth]
    return same_bytes(got[..., cols], want[..., cols]) and alpha_within_4_ulp(got[..., 25], want[..., 25])


def agree(got, want, smooth):
    """ a device result against the NumPy form's: ids, hits, state and covariance byte for byte, the rows too but for atan2's column """
    return (same_bytes(got[1], want[1]) and same_bytes(got[2], want[2]) and same_bytes(got[3], want[3]) and same_bytes(got[4], want[4])
            and rows_agree(got[0], want[0], smooth))


@pytest.mark.parametrize('name,frames,ego,opt', CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_host_form_and_the_oracle(name, frames, ego, opt):
    want = T.track_rows_np(frames, opt, ego=ego)
    oracle = K.track(frames, opt, ego)
    got = T.track_rows_device(frames, opt, ego=ego)
    assert len(got) == 5 and got[0].dtype == np.float32 and got[4].dtype == np.float64 and got[4].shape == (10, 128)
    assert agree(got, want, opt['smooth'])
    assert np.array_equal(got[1], oracle[1]) and np.array_equal(got[2], oracle[2]) and O.same_state(oracle[3], got[3]) and K.same_cov(oracle[4], got[4])
    assert (got[1] >= 0).sum() >= 16 and np.abs(got[4]).max() > 0.0
    if not opt['smooth']:
        assert same_bytes(got[0], frames)


@pytest.mark.parametrize('assign', T.ASSIGNS)
def test_the_demonstration_scene_on_the_device(assign):
    """ three identities under 'maha'; every fixed 'dist' threshold tears F or hands P's id to Q, in the same process """
    frames, gts = K.demo()
    opt = K.options('maha', assign=assign)
    got = T.track_rows_device(frames, opt)
    assert agree(got, T.track_rows_np(frames, opt), False)
    assert got[1][:, 0].tolist() == [0] * 12 and got[1][:, 1].tolist() == [1] * 6 + [2] * 6 and int(got[3]['next_id']) == 3
    assert T.id_switches(gts, got[1]) == 0
    for thr in K.DEMO_DIST:
        plain = O.options('dist', thr)
        ids = T.track_rows_device(frames, dict(plain, assign='optimal') if assign == 'optimal' else plain)[1]
        assert len(set(ids[:, 0].tolist())) > 1 or ids[5, 1] == ids[6, 1]


def device_chunks(frames, ego, opt, cuts):
    """ the sequence in calls of frames[cuts[k]:cuts[k + 1]] with their records, state and covariance carried on the device """
    dev = hip.require_device()
    state, cov = T.state_tensor(None, dev), T.cov_tensor(None, dev)
    rows, ids, hits = [], [], []
    for a, b in zip(cuts, cuts[1:]):
        r, i, h, state, cov = T.track_rows_device(torch.as_tensor(frames[a:b]).to(dev), opt, state, ego=None if ego is None else ego[a:b], cov=cov)
        rows.append(r.cpu().numpy()), ids.append(i.cpu().numpy()), hits.append(h.cpu().numpy())
    return np.concatenate(rows), np.concatenate(ids), np.concatenate(hits), state.cpu().numpy(), cov.cpu().numpy()


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('with_ego', [False, True])
def test_chunked_calls_give_the_same_bytes(with_ego, assign):
    """ 12 frames as one call, as twelve, and as (5, 7) """
    frames = K.DRIVE
    ego = K.ego_kinds(len(frames))['general'] if with_ego else None
    opt = K.options('maha', assign=assign, smooth=True)
    whole = device_chunks(frames, ego, opt, [0, 12])
    assert T.read_state(whole[3])['frames'] == 12 and same_bytes(T.read_cov(whole[4])[0], T.track_rows_np(frames, opt, ego=ego)[4])
    for cuts in (list(range(13)), [0, 5, 12]):
        for got, want in zip(device_chunks(frames, ego, opt, cuts), whole):
            assert same_bytes(got, want)


@pytest.mark.parametrize('assign', T.ASSIGNS)
def test_in_place(assign):
    """ rows_out == rows_in, state_out == state_in and cov_out == cov_in """
    frames = K.DRIVE
    ego = K.ego_kinds(len(frames))['general']
    opt = K.options('maha', assign=assign, smooth=True)
    want = T.track_rows_device(frames, opt, ego=ego)
    dev = hip.require_device()
    rows, state, cov = torch.as_tensor(frames).to(dev), T.state_tensor(None, dev), T.cov_tensor(None, dev)
    out, ids, hits, state_out, cov_out = T.track_rows_device(rows, opt, state, out=rows, state_out=state, ego=ego, cov=cov, cov_out=cov)
    assert out.data_ptr() == rows.data_ptr() and state_out.data_ptr() == state.data_ptr() and cov_out.data_ptr() == cov.data_ptr()
    assert same_bytes(rows.cpu().numpy(), want[0]) and same_bytes(ids.cpu().numpy(), want[1]) and same_bytes(hits.cpu().numpy(), want[2])
    assert same_bytes(T.read_state(state)[0], want[3]) and same_bytes(T.read_cov(cov)[0], want[4])


def test_nothing_to_do_copies_state_and_covariance():
    """ N = 0 and D = 0: GPP_OK, both are copied to their outputs """
    opt = K.options('maha')
    _, _, _, state, cov = T.track_rows_device(K.DRIVE[:3], opt)
    assert int(state['next_id']) > 0 and np.abs(cov).max() > 0.0
    for shape in ((0, 3, 36), (2, 0, 36)):
        rows, ids, hits, after, cov_after = T.track_rows_device(np.zeros(shape, np.float32), opt, state, cov=cov)
        assert rows.shape == shape and ids.shape == shape[:2] and same_bytes(after, state) and same_bytes(cov_after, cov)


@pytest.mark.parametrize('assign', T.ASSIGNS)
@pytest.mark.parametrize('metric', T.KF_METRICS)
def test_a_covariance_that_is_not_positive_definite_takes_the_fallback(metric, assign):
    """ tests/test_track_kf_cpu.py's scene: the kernel takes the branch the oracle and the NumPy form take """
    state, cov, frames, opt = H.fallback_scene(metric, assign)
    want = T.track_rows_np(frames, opt, state, cov=cov)
    got = T.track_rows_device(frames, opt, state, cov=cov)
    assert agree(got, want, False)
    assert got[1][0].tolist() == ([2, 1] if metric == 'maha' else [0, 1])
    if metric != 'maha':
        assert got[4][:, 0].tolist()[3:] == [0.0] * 4 + [4.0, 0.0, 4.0]


@pytest.mark.parametrize('metric,assign,records', H.CROWDS)
def test_one_crowded_frame(metric, assign, records):
    """ tests/track_crowd_cases.py's lattice of 128 x 128 cars that all overlap, behind quarter and half turns (optimal + ego + Kalman) and
    from a still camera (greedy + Kalman): frame 1 is 128 slots against 128 rows with every pair inside the gate -- the matrix beside A
    and R in LDS at its largest, every round of the greedy pass, a birth's covariance handed from the row's thread to the slot's in
    all 128 slots at once (frame 0) """
    frames, ego, opt = H.crowd(metric, assign, records)
    want = T.track_rows_np(frames, opt, ego=ego)
    assert (want[2][1] == 2).sum() == 128 and int(want[3]['next_id']) == 128 and (want[4][0] > 0.0).all()
    got = T.track_rows_device(frames, opt, ego=ego)
    assert agree(got, want, True)


def test_errors_return_their_code_and_write_nothing():
    """ the new errors of the contract, a short workspace and a misaligned covariance, on live device buffers full of a sentinel """
    dev = hip.require_device()
    frames = K.DRIVE[:3]
    N, D = frames.shape[:2]
    rows = torch.as_tensor(frames).to(dev)
    sbytes, cbytes = hip.track_state_bytes(), hip.track_cov_bytes()
    sentinel = lambda shape, dtype: torch.full(shape, 77, dtype=dtype, device=dev)  # noqa: E731
    out, ids, hits = sentinel((N, D, 36), torch.float32), sentinel((N, D), torch.int32), sentinel((N, D), torch.int32)
    state_in, state_out = torch.zeros((1, sbytes), dtype=torch.uint8, device=dev), sentinel((1, sbytes), torch.uint8)
    cov_in, cov_out = torch.zeros((1, cbytes + 8), dtype=torch.uint8, device=dev), sentinel((1, cbytes + 8), torch.uint8)
    work = torch.zeros((hip.track_ego_workspace_bytes(1, N),), dtype=torch.uint8, device=dev)
    opt = K.options('maha')
    params, kf = T.params_of(opt), T.kf_params_of(opt)
    seq = (ctypes.c_int32 * 2)(0, N)

    def call(work_bytes=len(work), k=kf, p=params, shift_in=0, shift_out=0, assign=0):
        return hip.lib().gpp_track_kf_f64(hip.ptr(rows), N, D, seq, 1, hip.ptr(state_in), hip.ptr(state_out), ctypes.c_void_p(cov_in.data_ptr() + shift_in),
                                          ctypes.c_void_p(cov_out.data_ptr() + shift_out), ctypes.byref(p), ctypes.byref(k), None, assign, hip.ptr(out), hip.ptr(ids),
                                          hip.ptr(hits), hip.ptr(work), work_bytes, hip.stream_ptr())

    assert call(len(work) - 8) == -2 and call(hip.track_workspace_bytes(1)) == -2        # the plain size is short, records or none
    assert call(shift_in=4) == -3 and call(shift_out=4) == -3
    assert call(k=hip.TrackKfParams(**dict(H.GOOD_KF, radial0=0.0))) == -1 and call(k=hip.TrackKfParams(**dict(H.GOOD_KF, reserved=1))) == -1
    assert call(p=hip.TrackParams(3, 2, 0, 0, float('inf'), 0.5, 0.25, 0.25, 0.0)) == -1 and call(assign=2) == -1
    torch.cuda.synchronize()
    for t in (out, ids, hits, state_out, cov_out):
        assert bool((t == 77).all())
    assert call() == 0                                                                    # the same buffers, a good call: it does write
    want = T.track_rows_np(frames, opt)
    assert same_bytes(ids.cpu().numpy(), want[1]) and same_bytes(T.read_state(state_out)[0], want[3])
    assert same_bytes(T.read_cov(cov_out[:, :cbytes].contiguous())[0], want[4])


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


MODEL_OPTION = {'metric': 'maha', 'threshold': 3.0, 'max_age': 1, 'smooth': True, 'filter': 'kalman', 'noise': K.NOISE}


def test_model_tracks_equal_the_host_form_over_its_pose_rows(weights50, monkeypatch):
    """ 2 + 2 frames through predict_tracks_on_frames against track_rows_np over the rows predict_poses_on_frames gives for the same four
    frames; track_covariance reads what belongs to track_state; reset_tracks zeroes both; a model without the filter has no covariance """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    model = models.load_model(weights50, backbone_name='resnet50', dtype='f32', pose=True, track=MODEL_OPTION)
    f = noise_frames(4, 96, 160, seed=5)
    P_inv, planes = calibration(2)
    assert int(model.track_state()['frames']) == 0 and not model.track_covariance().any()
    (rows_a, _, ids_a, hits_a), _ = model.predict_tracks_on_frames(f[:2], P_inv, planes)
    (pose_a, _), _ = model.predict_poses_on_frames(f[:2], P_inv, planes)
    (pose_b, _), _ = model.predict_poses_on_frames(f[2:], P_inv, planes)
    (rows_b, _, ids_b, hits_b), _ = model.predict_tracks_on_frames(f[2:], P_inv, planes)
    state, cov = model.track_state(), model.track_covariance()
    pose = np.concatenate([pose_a, pose_b])
    assert pose.shape == (4, 100, 36) and (pose[:, :, 14] >= 0).sum() >= 4                  # there is something to track
    want = T.track_rows_np(pose, MODEL_OPTION)
    got = (np.concatenate([rows_a, rows_b]), np.concatenate([ids_a, ids_b]), np.concatenate([hits_a, hits_b]), state, cov)
    assert agree(got, want, True) and int(state['frames']) == 4 and int(state['next_id']) > 0
    occupied = state['id1'] != 0
    assert occupied.any() and (cov[0][occupied] > 0.0).all() and not cov[:, ~occupied].any()
    model.reset_tracks()
    assert int(model.track_state()['frames']) == 0 and not model.track_covariance().any()
    (_, _, ids_c, hits_c), _ = model.predict_tracks_on_frames(f[:2], P_inv, planes)
    assert same_bytes(ids_c, ids_a) and same_bytes(hits_c, hits_a)
    plain = models.load_model(weights50, backbone_name='resnet50', dtype='f32', pose=True, track=('dist', 6.0))
    with pytest.raises(hip.GppError, match='no covariance'):
        plain.track_covariance()


def test_range_event_advances_state_and_covariance_once(weights50, monkeypatch):
    """ the weights of tests/test_track_gpu.py's range event: the float32 twin answers the call; the reader has then run twice, and state
    and covariance have advanced once, by the twin's rows; the next call continues from both """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    B, h, w = 2, 96, 160
    scaled = dict(weights50)
    k = np.float32(2.0 ** 17)
    scaled['bn2a_branch2a/gamma'], scaled['bn2a_branch2a/beta'] = scaled['bn2a_branch2a/gamma'] * k, scaled['bn2a_branch2a/beta'] * k
    scaled['res2a_branch2b/kernel'] = scaled['res2a_branch2b/kernel'] / k
    option = dict(MODEL_OPTION, smooth=False)
    tracked = models.load_model(scaled, backbone_name='resnet50', dtype='f16x3', pose=True, track=option)
    m32 = models.load_model(scaled, backbone_name='resnet50', dtype='f32', pose=True)
    P_inv, planes = calibration(B)
    x = np.random.default_rng(0).integers(0, 256, size=(B, h, w, 3)).astype(np.float32) - MEAN
    inputs = [x, P_inv, planes]
    rows, counts, ids, hits = tracked.predict_tracks_on_batch(inputs, 1.25, (h, w, 3))
    assert tracked.range_fallbacks == 1
    want_rows, _ = m32.predict_poses_on_batch(inputs, 1.25, (h, w, 3))
    assert same_bytes(rows, want_rows)
    want = T.track_rows_np(want_rows, option)
    state, cov = tracked.track_state(), tracked.track_covariance()
    assert int(state['frames']) == B and same_bytes(state, want[3]) and same_bytes(cov, want[4]) and same_bytes(ids, want[1])
    assert np.abs(cov).max() > 0.0
    _, _, ids2, hits2 = tracked.predict_tracks_on_batch(inputs, 1.25, (h, w, 3))
    want2 = T.track_rows_np(want_rows, option, want[3], cov=want[4])
    assert tracked.range_fallbacks == 2 and same_bytes(ids2, want2[1]) and same_bytes(hits2, want2[2])
    assert same_bytes(tracked.track_state(), want2[3]) and same_bytes(tracked.track_covariance(), want2[4]) and int(want2[3]['frames']) == 2 * B


def test_command_lines_write_the_host_forms_tracks(weights50, tmp_path, monkeypatch):
    """ bin/track_results.py with the filter's arguments on the demonstration scene's result files: the device writes the bytes --host
    writes; bin/run_network.py --track maha --track-filter kalman ... against tracking_lines over track_rows_np of the rows its calls
    returned """
    from PIL import Image
    from keras_retinanet_3D.bin import run_network, track_results
    from keras_retinanet_3D.models import retinanet
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    H.write_results(str(tmp_path / 'kitti'), K.demo()[0])
    common = [str(tmp_path / 'kitti'), '--metric', 'maha', '--threshold', '3'] + H.KALMAN_ARGS
    track_results.main([common[0], str(tmp_path / 'device.txt')] + common[1:])
    track_results.main([common[0], str(tmp_path / 'host.txt')] + common[1:] + ['--host'])
    text = (tmp_path / 'device.txt').read_text()
    assert text == (tmp_path / 'host.txt').read_text() and sorted({int(line.split()[1]) for line in text.splitlines()}) == [0, 1, 2]
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
                      '--kitti', '--batch-size', '2', '--device-pose', '--track', 'maha', '--track-threshold', '3', '--track-max-age', '1'] + H.KALMAN_ARGS)
    assert [s[0].shape[0] for s in seen] == [2, 1]
    rows = np.concatenate([s[0] for s in seen])
    _, ids, hits, _, _ = T.track_rows_np(rows, dict(K.options('maha'), max_age=1))
    assert same_bytes(ids, np.concatenate([s[2] for s in seen])) and (ids >= 0).sum() >= 3
    want = ''.join(T.tracking_lines(k, rows[k], ids[k], hits[k]) for k in range(3))
    assert (tmp_path / 'out' / 'synthetic:1234' / 'outputs' / 'tracking' / 'tracks.txt').read_text() == want
