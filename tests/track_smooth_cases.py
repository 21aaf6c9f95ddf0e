""" Scenes of the offline smoother's tests, shared by tests/test_track_smooth_cpu.py and tests/test_track_smooth_gpu.py:
finished runs -- raw rows (N, D, 36) and the tracker's ids (N, D) -- written down directly, without a tracker in between. """
import math
import os

import numpy as np

import track_ego_oracle as E
import track_kf_oracle as K
from track_oracle import padding, row
from keras_retinanet_3D.utils import gpp_utils

NOISE = K.NOISE


def general_yaw(angle=0.04, t=(0.125, -0.03125, -1.5)):
    """ a record that turns about the camera's Y axis only (R01 = R21 = 0) and shifts """
    return E.record(E.rot_y(angle)[:3, :3], t, angle)


def records(kind, N):
    """ (N, 16) records: 'identity', 'turns' (quarter and half turns with dyadic shifts), 'yaw' (a general yaw in every frame) or
    'general' (yaw and pitch in frame 1, a general yaw elsewhere); None for None """
    if kind is None:
        return None
    if kind == 'identity':
        return np.array(E.cycle([E.IDENTITY], N))
    if kind == 'turns':
        return np.array(E.cycle(E.TURNS, N))
    if kind == 'yaw':
        return np.array([general_yaw(0.04 if f % 2 else -0.03, (0.125 * (f % 3), 0.0, -1.5)) for f in range(N)])
    return np.array([K.general_record() if f == 1 else general_yaw() for f in range(N)])


def scene(seed, N, D, cars, miss=0.25, seq_start=None, spread=1.0):
    """ `cars` identities per sequence, each alive over a random stretch of its sequence and missed with probability `miss` per frame, at
    random rows of their frames; noisy positions along a straight path, r_y anywhere in [-pi, pi) -> (rows (N, D, 36), ids (N, D)) """
    rng = np.random.default_rng(seed)
    rows = np.stack([padding(D) for _ in range(N)])
    ids = np.full((N, D), -1, np.int32)
    used = np.zeros(N, np.int64)
    bounds = [0, N] if seq_start is None else list(seq_start)
    for s in range(len(bounds) - 1):
        lo, hi = bounds[s], bounds[s + 1]
        for car in range(cars):
            a = int(rng.integers(lo, max(lo + 1, hi - 1)))
            b = int(rng.integers(a + 1, hi + 1)) if rng.random() < 0.8 else a + 1
            x0, z0 = rng.uniform(-12.0, 12.0), rng.uniform(8.0, 60.0)
            vx, vz = rng.normal(0.0, 0.2), rng.normal(0.0, 0.8)
            ry = rng.uniform(-math.pi, math.pi)
            for f in range(a, b):
                if rng.random() < miss or used[f] >= D:
                    continue
                k = f - a
                r = row(rng.uniform(0.1, 1.0), x0 + vx * k + spread * rng.normal(0.0, 0.3), z0 + vz * k + spread * rng.normal(0.0, 1.0),
                        ry=float((ry + rng.normal(0.0, 0.1) + (math.pi if rng.random() < 0.1 else 0.0) + math.pi) % (2.0 * math.pi) - math.pi),
                        h=rng.uniform(1.4, 1.8), y=1.65 + rng.normal(0.0, 0.05), orient=int(rng.integers(0, 4)))
                r[0:4] += np.float32(k)
                r[26:30] += np.float32(k)
                rows[f, used[f]], ids[f, used[f]] = r, car
                used[f] += 1
    for f in range(N):                                                    # the rows of a frame in random order
        p = rng.permutation(D)
        rows[f], ids[f] = rows[f][p], ids[f][p]
    return rows, ids


def chains(n_seg, length, D=None, step=1):
    """ n_seg identities, each detected at `length` cells `step` frames apart from frame 0 on (step - 1 gaps between two detections) """
    N = (length - 1) * step + 1
    D = n_seg if D is None else D
    rows = np.stack([padding(D) for _ in range(N)])
    ids = np.full((N, D), -1, np.int32)
    for k in range(n_seg):
        for c in range(length):
            f = c * step
            rows[f, k] = row(0.5, -20.0 + 0.5 * k + 0.01 * c * (k % 5), 10.0 + 0.3 * k + 0.5 * c + 0.2 * ((c + k) % 3), ry=0.1 * k - 3.0 + 0.05 * c,
                             orient=k % 4)
            ids[f, k] = k
    return rows, ids


def receding(seed, frames=40, miss=0.2, noise=NOISE):
    """ the issue's scene: one car receding from 15 m at a constant velocity under the noise model itself, `miss` of the frames missed ->
    (rows (frames, 1, 36), ids (frames, 1), truth (frames, 2)) """
    rng = np.random.default_rng(seed)
    truth = np.stack([1.5 + 0.05 * np.arange(frames), 15.0 + 0.9 * np.arange(frames)], axis=1)
    rows = np.stack([padding(1) for _ in range(frames)])
    ids = np.full((frames, 1), -1, np.int32)
    for f in range(frames):
        if 0 < f < frames - 1 and rng.random() < miss:
            continue
        x, z = truth[f]
        rho = math.hypot(x, z)
        along = rng.normal(0.0, noise['radial'][0] + noise['radial'][1] * rho)
        across = rng.normal(0.0, noise['tangential'][0] + noise['tangential'][1] * rho)
        ux, uz = x / rho, z / rho
        rows[f, 0] = row(0.9, x + along * ux + across * uz, z + along * uz - across * ux)
        ids[f, 0] = 0
    return rows, ids, truth


def same_outputs(got, want):
    """ every word ==; column 25 (an atan2) within 4 float32 ulp, section 4.28's bar """
    cols = [c for c in range(36) if c != 25]
    for g, w in ((got[0], want[0]), (got[2], want[2])):
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(g[..., cols], w[..., cols], equal_nan=True)
        a, b = g[..., 25].astype(np.float64), w[..., 25].astype(np.float64)
        assert ((np.abs(a - b) <= 4 * np.spacing(np.abs(w[..., 25]))) | (a == b) | (np.isnan(a) & np.isnan(b))).all()
    for g, w in ((got[1], want[1]), (got[3], want[3])):
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w, equal_nan=True)


KALMAN = ['--track-noise', '0.1', '0.05', '0.1', '0.005', '--track-process', '0.01', '0.01', '--track-birth-speed', '2']


def write_run(tmp_path, missed=(3, 5)):
    """ one car in 8 frames, its box fixed in the image, as KITTI result files with the frames `missed` empty, and its labels """
    os.mkdir(str(tmp_path / 'kitti'))
    for f in range(8):
        rows = np.stack([row(0.9, 1.0 + 0.25 * f, 20.0 + 0.5 * f + 0.125 * (f % 2))]) if f not in missed else padding(1)
        with open(str(tmp_path / 'kitti' / ('%06d.txt' % f)), 'w') as out:
            out.write(gpp_utils.kitti_lines_from_rows(rows, int((rows[:, 14] >= 0).sum())))
    (tmp_path / 'l.txt').write_text(''.join('{} 4 Car 0 0 0.25 100 100 200 180 1.5 2 3 {} 1.65 {} 0\n'.format(f, 1.0 + 0.25 * f, 20.0 + 0.5 * f)
                                            for f in range(8)))
    return [str(tmp_path / 'kitti'), str(tmp_path / 'tracks.txt'), '--metric', 'dist', '--threshold', '3', '--host']
