""" CPU tests of utils/oxts.py: camera poses from KITTI's oxts and calibration files.  Neither the devkit nor an
oxts file is part of this repository: what is tested is self-consistency.  A synthetic oxts file, written here from a known planar
trajectory through the INVERSE of the devkit's Mercator projection (written out below, not imported), must come back as that trajectory;
camera_ego against hand-computed transforms; the commands' line-count check.  Every fixture is written into tmp_path. """
import math

import numpy as np
import pytest

from keras_retinanet_3D.utils import oxts
from keras_retinanet_3D.utils import track as T

ER = 6378137.0
LAT0, LON0, ALT0, YAW0 = 49.011212804408, 8.4228850417969, 112.834, 0.3757       # (about where KITTI was driven)


def planar_trajectory(n=12):
    """ n poses in the first frame's IMU coordinates (x forward, y left, z up): 1.5 m per frame, 0.04 rad of yaw per frame
    -> x, y, z, yaw (n,) """
    x, y, yaw = np.zeros(n), np.zeros(n), 0.04 * np.arange(n)
    for f in range(1, n):
        x[f], y[f] = x[f - 1] + 1.5 * math.cos(yaw[f - 1]), y[f - 1] + 1.5 * math.sin(yaw[f - 1])
    return x, y, 0.01 * np.arange(n), yaw


def write_oxts(path, x, y, z, yaw, roll=0.0, pitch=0.0):
    """ the trajectory as an oxts file: into the world's Mercator metres by the first frame's pose (LAT0, LON0, YAW0), then through the
    inverse projection: lon = mx 180 / (scale pi er), lat = 360 / pi atan(exp(my / (scale er))) - 90, scale = cos(LAT0 pi / 180) """
    scale = math.cos(LAT0 * math.pi / 180.0)
    mx0 = scale * LON0 * math.pi * ER / 180.0
    my0 = scale * ER * math.log(math.tan((90.0 + LAT0) * math.pi / 360.0))
    lines = []
    for f in range(len(x)):
        mx = mx0 + math.cos(YAW0) * x[f] - math.sin(YAW0) * y[f]
        my = my0 + math.sin(YAW0) * x[f] + math.cos(YAW0) * y[f]
        lon = mx * 180.0 / (scale * math.pi * ER)
        lat = 360.0 / math.pi * math.atan(math.exp(my / (scale * ER))) - 90.0
        words = [lat, lon, ALT0 + z[f], roll, pitch, YAW0 + yaw[f]] + [0.0] * 17 + [0.05, 0.01, 4, 10, 4, 4, 4]
        lines.append(' '.join(repr(float(w)) if k < 25 else str(int(w)) for k, w in enumerate(words)))
    path.write_text('\n'.join(lines) + '\n')


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def test_a_synthetic_oxts_file_comes_back_as_its_trajectory(tmp_path):
    """ within 1e-6 m and 1e-9 rad.  The bar: the Mercator coordinates are about 4e6 m, where a float64 is 1e-9 m apart; the projection,
    its inverse and the pose product are a few dozen operations, so the positions agree to some 1e-8 m, and the file carries 17 digits.
    The angles go through cos / sin and one 3 x 3 product: 1e-15 rad """
    x, y, z, yaw = planar_trajectory()
    write_oxts(tmp_path / '0000.txt', x, y, z, yaw)
    rows = oxts.read_oxts(str(tmp_path / '0000.txt'))
    assert rows.shape == (12, 30) and rows.dtype == np.float64 and abs(rows[0, 0] - LAT0) < 1e-12 and rows[3, 25] == 4.0
    poses = oxts.poses_from_oxts(rows)
    assert poses.shape == (12, 4, 4) and np.abs(poses[0] - np.eye(4)).max() < 1e-9 and (poses[:, 3] == [0.0, 0.0, 0.0, 1.0]).all()
    assert np.abs(poses[:, 0, 3] - x).max() < 1e-6 and np.abs(poses[:, 1, 3] - y).max() < 1e-6 and np.abs(poses[:, 2, 3] - z).max() < 1e-6
    print('position error', np.abs(poses[:, :2, 3] - np.stack([x, y], axis=1)).max())
    for f in range(12):
        assert np.abs(poses[f, :3, :3] - rot_z(yaw[f])).max() < 1e-9
        assert abs(math.atan2(poses[f, 1, 0], poses[f, 0, 0]) - yaw[f]) < 1e-9


def test_roll_and_pitch_follow_the_devkit_s_order(tmp_path):
    """ R = Rz(yaw) Ry(pitch) Rx(roll): the pose of frame 1 relative to frame 0 with the same roll and pitch in both """
    x, y, z, yaw = planar_trajectory(2)
    write_oxts(tmp_path / 'o.txt', x, y, z, yaw, roll=0.02, pitch=-0.03)
    poses = oxts.poses_from_oxts(oxts.read_oxts(str(tmp_path / 'o.txt')))
    cr, sr, cp, sp = math.cos(0.02), math.sin(0.02), math.cos(-0.03), math.sin(-0.03)
    tilt = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]]).dot(np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]]))
    want = tilt.T.dot(rot_z(0.04)).dot(tilt)                                       # inv(Rz(a) T) Rz(a + 0.04) T
    assert np.abs(poses[1, :3, :3] - want).max() < 1e-9
    assert np.abs(poses[1, :3, 3] - tilt.T.dot([1.5, 0.0, 0.01])).max() < 1e-6


def test_read_oxts_refuses_a_short_line(tmp_path):
    (tmp_path / 'o.txt').write_text(' '.join(['0.0'] * 30) + '\n\n' + ' '.join(['0.0'] * 29) + '\n')
    with pytest.raises(ValueError, match='line 3 has 29 numbers'):
        oxts.read_oxts(str(tmp_path / 'o.txt'))
    assert oxts.poses_from_oxts(np.zeros((0, 30))).shape == (0, 4, 4)


IDENTITY_CALIB = ('P0: 1 0 0 0 0 1 0 0 0 0 1 0\nR_rect 1 0 0 0 1 0 0 0 1\nTr_velo_cam 1 0 0 0 0 1 0 0 0 0 1 0\n'
                  'Tr_imu_velo 1 0 0 0 0 1 0 0 0 0 1 0\n')
# velodyne (x forward, y left, z up) -> camera (x right, y down, z forward): x_c = -y_v, y_c = -z_v, z_c = x_v; the offsets are dyadic
SWAP_CALIB = ('R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0.5 0 0 -1 -0.25 1 0 0 -1.0\nTr_imu_to_velo: 1 0 0 0.75 0 1 0 0 0 0 1 0.125\n')


def test_read_tracking_calibration_takes_both_spellings(tmp_path):
    (tmp_path / 'a.txt').write_text(IDENTITY_CALIB)
    (tmp_path / 'b.txt').write_text(SWAP_CALIB)
    a, b = oxts.read_tracking_calibration(str(tmp_path / 'a.txt')), oxts.read_tracking_calibration(str(tmp_path / 'b.txt'))
    assert sorted(a) == sorted(b) == ['R_rect', 'Tr_imu_velo', 'Tr_velo_cam']
    assert all(np.array_equal(a[k], np.eye(4)) for k in a)
    assert b['Tr_velo_cam'].tolist() == [[0, -1, 0, 0.5], [0, 0, -1, -0.25], [1, 0, 0, -1.0], [0, 0, 0, 1]]
    assert b['Tr_imu_velo'][:3, 3].tolist() == [0.75, 0.0, 0.125]
    (tmp_path / 'c.txt').write_text('R_rect 1 0 0 0 1 0 0 0 1\nTr_velo_cam 1 0 0 0 0 1 0 0 0 0 1 0\n')
    with pytest.raises(ValueError, match='no Tr_imu_velo'):
        oxts.read_tracking_calibration(str(tmp_path / 'c.txt'))
    (tmp_path / 'd.txt').write_text('R_rect 1 0 0 0 1 0 0 0\n')
    with pytest.raises(ValueError, match='R_rect has 8 numbers'):
        oxts.read_tracking_calibration(str(tmp_path / 'd.txt'))


def compose(records):
    """ the records one after the other, as 4 x 4: E_f ... E_1 E_0 """
    out, total = [], np.eye(4)
    for r in records:
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = r[:9].reshape(3, 3), r[9:12]
        total = E.dot(total)
        out.append(total)
    return np.stack(out)


def test_camera_ego_with_the_identity_calibration(tmp_path):
    """ the camera is the IMU: record f is inv(pose_f) pose_(f-1), frame 0 the identity, and the records composed give inv(pose_f) pose_0 """
    x, y, z, yaw = planar_trajectory()
    write_oxts(tmp_path / 'o.txt', x, y, z, yaw)
    (tmp_path / 'c.txt').write_text(IDENTITY_CALIB)
    poses = oxts.poses_from_oxts(oxts.read_oxts(str(tmp_path / 'o.txt')))
    rec = oxts.camera_ego(poses, oxts.read_tracking_calibration(str(tmp_path / 'c.txt')))
    assert rec.shape == (12, 16) and rec[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0] and T.check_ego(rec, 12) is not None
    assert rec.tobytes() == oxts.camera_ego(poses).tobytes()
    for f in range(1, 12):                             # by hand: the IMU turned 0.04 rad about z and drove 1.5 m along its old x
        assert np.abs(rec[f, :9].reshape(3, 3) - rot_z(-0.04)).max() < 1e-9
        assert np.abs(rec[f, 9:12] - rot_z(-0.04).dot([-1.5, 0.0, -0.01])).max() < 1e-6
    total = compose(rec)
    for f in range(12):
        assert np.abs(total[f] - np.linalg.inv(poses[f]).dot(poses[0])).max() < 1e-9


def test_camera_ego_with_swapped_axes(tmp_path):
    """ velodyne axes -> camera axes: the car's left turn by 0.04 rad (about the IMU's z, which points up) carries the points of the old
    camera coordinates by a turn of +0.04 rad about the camera's Y, which points down -- dyaw = +0.04, a parked car's r_y grows.  The
    transforms are computed by hand below from C = Tr_velo_cam Tr_imu_velo """
    x, y, z, yaw = planar_trajectory()
    write_oxts(tmp_path / 'o.txt', x, y, z, yaw)
    (tmp_path / 'c.txt').write_text(SWAP_CALIB)
    poses = oxts.poses_from_oxts(oxts.read_oxts(str(tmp_path / 'o.txt')))
    rec = oxts.camera_ego(poses, oxts.read_tracking_calibration(str(tmp_path / 'c.txt')))
    # by hand: C p = A p + c with A = [[0, -1, 0], [0, 0, -1], [1, 0, 0]], c = A (0.75, 0, 0.125) + (0.5, -0.25, -1) = (0.5, -0.375, -0.25);
    # the IMU step is p -> Rz(-0.04) (p - d), d = (1.5, 0, 0.01); so the camera step is q -> A Rz(-0.04) A' (q - c) - A Rz(-0.04) d + c
    A, c, d = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]), np.array([0.5, -0.375, -0.25]), np.array([1.5, 0.0, 0.01])
    R = A.dot(rot_z(-0.04)).dot(A.T)
    cs, sn = math.cos(0.04), math.sin(0.04)
    assert np.abs(R - np.array([[cs, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, cs]])).max() < 1e-15      # a turn by +0.04 about the camera's Y
    t = c - R.dot(c) - A.dot(rot_z(-0.04)).dot(d)
    for f in range(1, 12):
        assert np.abs(rec[f, :9].reshape(3, 3) - R).max() < 1e-9 and np.abs(rec[f, 9:12] - t).max() < 1e-6
        assert abs(rec[f, 12] - 0.04) < 1e-9
    # a parked car 20 m ahead and 4 m to the right of camera 0 comes 1.5 m nearer per frame
    p = compose(rec)[:, :3, :].dot([4.0, 1.65, 20.0, 1.0])
    assert abs(p[1][2] - 20.0 + 1.5) < 0.2 and (np.diff(p[:, 2]) < -1.0).all()
    C = oxts.camera_from_imu(oxts.read_tracking_calibration(str(tmp_path / 'c.txt')))
    total = compose(rec)
    for f in range(12):
        assert np.abs(total[f] - C.dot(np.linalg.inv(poses[f])).dot(poses[0]).dot(np.linalg.inv(C))).max() < 1e-9


def test_the_records_track_what_the_file_describes(tmp_path):
    """ end to end on the host: cars parked in the world, seen from the camera of the synthetic file, keep their ids with the file's
    records and do not without them """
    x, y, z, yaw = planar_trajectory()
    write_oxts(tmp_path / 'o.txt', x, y, z * 0.0, yaw)
    (tmp_path / 'c.txt').write_text(SWAP_CALIB)
    rec = oxts.records_for(str(tmp_path / 'o.txt'), str(tmp_path / 'c.txt'), 12)
    total = compose(rec)
    cars = np.array([[4.0 if k % 2 else -4.0, 1.65, 10.0 + 4.0 * k, 1.0] for k in range(8)])
    frames = np.full((12, 8, 36), -1.0, np.float32)
    for f in range(12):
        p = total[f].dot(cars.T).T
        frames[f, :, 12], frames[f, :, 14] = 0.9, 0.0
        frames[f, :, 19], frames[f, :, 31], frames[f, :, 21] = p[:, 0], p[:, 1], p[:, 2]
        frames[f, :, 32], frames[f, :, 30], frames[f, :, 17], frames[f, :, 18] = rec[:f + 1, 12].sum(), 1.5, 1.6, 4.0
    opt = ('dist', 1.0)
    assert int(T.track_rows_np(frames, opt)[3]['next_id']) > 8
    state = T.track_rows_np(frames, opt, ego=rec)[3]
    assert int(state['next_id']) == 8 and np.abs(state['box'][7:10]).max() < 1e-5


def test_a_wrong_line_count_is_refused_and_names_both_counts(tmp_path):
    from keras_retinanet_3D.bin import run_network, track_results
    x, y, z, yaw = planar_trajectory(3)
    write_oxts(tmp_path / 'o.txt', x, y, z, yaw)
    (tmp_path / 'c.txt').write_text(IDENTITY_CALIB)
    assert oxts.records_for(str(tmp_path / 'o.txt'), str(tmp_path / 'c.txt'), 3).shape == (3, 16)
    with pytest.raises(ValueError, match='has 3 lines for 4 images'):
        oxts.records_for(str(tmp_path / 'o.txt'), str(tmp_path / 'c.txt'), 4)
    # track_results.py --host: two result files against three oxts lines, then the right count; without the options the bytes of before
    line = 'Car -1 -1 0.25 100.00 100.00 200.00 180.00 1.50 2.00 3.00 {:.3f} 1.65 {:.2f} 0.00 {:.2f}\n'
    (tmp_path / 'r').mkdir()
    (tmp_path / 'r' / '000000.txt').write_text(line.format(0.0, 20.0, 0.9))
    (tmp_path / 'r' / '000001.txt').write_text(line.format(0.0, 18.5, 0.9))
    run = [str(tmp_path / 'r'), str(tmp_path / 't.txt'), '--metric', 'dist', '--threshold', '1', '--host']
    with pytest.raises(ValueError, match='has 3 lines for 2 images'):
        track_results.main(run + ['--oxts', str(tmp_path / 'o.txt'), '--calib', str(tmp_path / 'c.txt')])
    track_results.main(run)
    plain = (tmp_path / 't.txt').read_text()
    assert [ln.split()[:2] for ln in plain.splitlines()] == [['0', '0'], ['1', '1']]       # 1.5 m nearer: another car to the plain tracker
    write_oxts(tmp_path / 'o2.txt', x[:2], y[:2], z[:2] * 0.0, yaw[:2] * 0.0)     # 1.5 m along the IMU's x: the camera's z under the swap
    (tmp_path / 'c2.txt').write_text(SWAP_CALIB)
    track_results.main(run + ['--oxts', str(tmp_path / 'o2.txt'), '--calib', str(tmp_path / 'c2.txt')])
    assert [ln.split()[:2] for ln in (tmp_path / 't.txt').read_text().splitlines()] == [['0', '0'], ['1', '0']]
    track_results.main(run)
    assert (tmp_path / 't.txt').read_text() == plain
    with pytest.raises(SystemExit):
        track_results.parse_args(run + ['--oxts', 'o.txt'])
    # run_network.py: the options' own checks and the model option they make
    base = ['m.h5', 'img', 'calib', 'planes.mat', 'out', '--device-pose', '--track', 'dist', '--track-threshold', '2']
    args = run_network.parse_args(base + ['--track-oxts', 'o.txt', '--track-calib', 'c.txt'])
    assert run_network.track_option(args) == {'metric': 'dist', 'threshold': 2.0, 'max_age': 2, 'smooth': False, 'ego': True}
    assert run_network.track_option(run_network.parse_args(base)) == {'metric': 'dist', 'threshold': 2.0, 'max_age': 2, 'smooth': False}
    for bad in (base + ['--track-oxts', 'o.txt'], base + ['--track-calib', 'c.txt'],
                base[:5] + ['--device-pose', '--track-oxts', 'o.txt', '--track-calib', 'c.txt']):
        with pytest.raises(SystemExit):
            run_network.parse_args(bad)
