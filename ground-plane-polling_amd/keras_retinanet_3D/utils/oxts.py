"""
Camera poses from KITTI's GPS/IMU files: the ego records of the tracker (utils/track.py, gpp_track_ego_f64) from the
`oxts/<seq>.txt` and `calib/<seq>.txt` that KITTI tracking ships beside the images.

    read_oxts                   30 numbers per line, one line per frame
    poses_from_oxts             a restatement of the raw-data devkit's convertOxtsToPose.m: IMU poses relative to the first frame
    read_tracking_calibration   R_rect, Tr_velo_cam, Tr_imu_velo as 4 x 4
    camera_ego                  per frame the transform from the previous frame's rectified camera coordinates to this frame's -> records
    records_for                 the two files of a sequence -> the (N, 16) records of its N images

Parity with the devkit itself is UNPINNED: neither the devkit nor an oxts file is part of this repository; what is tested is
self-consistency (tests/test_oxts_cpu.py: a synthetic file written through the inverse projection comes back as the trajectory it was
made from).  All of it is float64 NumPy on the host -- a few hundred bytes per frame; there is no kernel.
"""
import numpy as np

from . import track

OXTS_COLUMNS = 30                           # lat lon alt roll pitch yaw vn ve vf vl vu ax ay az af al au wx wy wz wf wl wu pos_acc vel_acc navstat numsats posmode velmode orimode
EARTH_RADIUS = 6378137.0                    # metres, the devkit's `er`


def read_oxts(path):
    """ an oxts file -> (N, 30) float64: one line per frame, 30 numbers per line (empty lines are skipped) """
    rows = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            words = line.split()
            if not words:
                continue
            if len(words) != OXTS_COLUMNS:
                raise ValueError('{}: line {} has {} numbers, an oxts line has {}'.format(path, number, len(words), OXTS_COLUMNS))
            rows.append([float(w) for w in words])
    return np.array(rows, np.float64).reshape(-1, OXTS_COLUMNS)


def poses_from_oxts(oxts):
    """ (N, 30) oxts rows -> (N, 4, 4) float64: the IMU's pose in the coordinates of the first frame's IMU (the first is the identity).
    convertOxtsToPose.m, restated: the Mercator scale is cos(latitude of the FIRST frame); x = scale lon pi er / 180, y = scale er
    log(tan((90 + lat) pi / 360)), z = alt; R = Rz(yaw) Ry(pitch) Rx(roll); pose_f = inv(T_0) T_f """
    oxts = np.asarray(oxts, np.float64).reshape(-1, OXTS_COLUMNS)
    if oxts.shape[0] == 0:
        return np.zeros((0, 4, 4))
    lat, lon, alt, roll, pitch, yaw = [oxts[:, k] for k in range(6)]
    scale = np.cos(lat[0] * np.pi / 180.0)
    T = np.zeros((oxts.shape[0], 4, 4))
    T[:, 0, 3] = scale * lon * np.pi * EARTH_RADIUS / 180.0
    T[:, 1, 3] = scale * EARTH_RADIUS * np.log(np.tan((90.0 + lat) * np.pi / 360.0))
    T[:, 2, 3] = alt
    T[:, 3, 3] = 1.0
    cx, sx, cy, sy, cz, sz = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    zero, one = np.zeros_like(cx), np.ones_like(cx)
    Rx = np.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], axis=1).reshape(-1, 3, 3)
    Ry = np.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], axis=1).reshape(-1, 3, 3)
    Rz = np.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], axis=1).reshape(-1, 3, 3)
    T[:, :3, :3] = np.matmul(Rz, np.matmul(Ry, Rx))
    return np.matmul(rigid_inverse(T[0]), T)


def rigid_inverse(T):
    """ the inverse of a rigid 4 x 4 transform [R t; 0 1]: [R' -R' t; 0 1] (no general inverse: the translations are 1e6 m) """
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    R = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = R
    out[..., :3, 3] = -np.matmul(R, T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def read_tracking_calibration(path):
    """ a calibration file -> {'R_rect', 'Tr_velo_cam', 'Tr_imu_velo'}: 4 x 4 float64.  Both spellings of the keys are taken: the tracking
    benchmark's (R_rect, Tr_velo_cam, Tr_imu_velo) and the object benchmark's (R0_rect, Tr_velo_to_cam, Tr_imu_to_velo), with or without
    a colon behind the key """
    names = {'R_rect': 'R_rect', 'R0_rect': 'R_rect', 'Tr_velo_cam': 'Tr_velo_cam', 'Tr_velo_to_cam': 'Tr_velo_cam',
             'Tr_imu_velo': 'Tr_imu_velo', 'Tr_imu_to_velo': 'Tr_imu_velo'}
    out = {}
    with open(path) as f:
        for line in f:
            words = line.split()
            if not words or words[0].rstrip(':') not in names:
                continue
            key = names[words[0].rstrip(':')]
            values = np.array([float(w) for w in words[1:]], np.float64)
            if values.size != (9 if key == 'R_rect' else 12):
                raise ValueError('{}: {} has {} numbers, expected {}'.format(path, words[0], values.size, 9 if key == 'R_rect' else 12))
            M = np.eye(4)
            if key == 'R_rect':
                M[:3, :3] = values.reshape(3, 3)
            else:
                M[:3, :4] = values.reshape(3, 4)
            out[key] = M
    missing = sorted(set(names.values()) - set(out))
    if missing:
        raise ValueError('{}: no {} (nor the object benchmark\'s spelling of it)'.format(path, ', '.join(missing)))
    return out


def camera_from_imu(calib):
    """ R_rect . Tr_velo_cam . Tr_imu_velo: an IMU point -> rectified camera metres (the coordinates of the pose rows) """
    return calib['R_rect'].dot(calib['Tr_velo_cam']).dot(calib['Tr_imu_velo'])


def camera_ego(oxts_poses, calib=None):
    """ poses_from_oxts' (N, 4, 4) and read_tracking_calibration's dict (None: the camera is the IMU) -> the (N, 16) records of
    utils/track.ego_records: record f carries a point from the rectified camera coordinates of frame f - 1 into those of frame f,
    C inv(pose_f) pose_(f-1) inv(C) with C = camera_from_imu; frame 0 is the identity """
    poses = np.asarray(oxts_poses, np.float64).reshape(-1, 4, 4)
    C = np.eye(4) if calib is None else camera_from_imu(calib)
    out = np.tile(np.eye(4), (poses.shape[0], 1, 1))
    if poses.shape[0] > 1:
        step = np.matmul(rigid_inverse(poses[1:]), poses[:-1])                  # IMU f from IMU f - 1
        out[1:] = np.matmul(C, np.matmul(step, np.linalg.inv(C)))               # (a file's R_rect is orthonormal to its printed digits only)
    return track.ego_records(out)


def records_for(oxts_path, calib_path, images):
    """ the records of a sequence of `images` images: one oxts line per image of the sorted list -- any other count is an error that
    names both """
    oxts = read_oxts(oxts_path)
    if oxts.shape[0] != int(images):
        raise ValueError('{} has {} lines for {} images: one oxts line per image of the sorted list'.format(oxts_path, oxts.shape[0], int(images)))
    return camera_ego(poses_from_oxts(oxts), read_tracking_calibration(calib_path))
