"""
ORACLE of the device pose stage (csrc/pose.hip): a float64 restatement, one detection at a time, of what the reference's
bin/run_network.py does with the 8 model outputs of one image (/root/reference/keras_retinanet_3D/bin/run_network.py:113-330):
scale correction and selection (:113-135), 6-DoF pose from the 3-D keypoints (:137-247, the two live `outlier` branches), cuboid
corners and the KITTI fields (:298-330).  Both Rodrigues directions are oracle.pose_np.rodrigues, the scalar stand-in for
cv2.Rodrigues that tests/test_harness.py checks the host path with.  Nothing of utils.gpp_utils is called here.

The reference keeps its intermediate results in float32 arrays; here every float32 input is widened once and every step is float64,
so that the deviation of a float32 implementation (the host path of utils.gpp_utils, the rows of gpp_pose_f32) can be measured
against it.
"""
import math

import numpy as np

from oracle import pose_np

COLS = 36
KITTI_FORMAT = "Car -1 -1 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n"
# row layout (include/gpp.h, gpp_pose_f32)
BOX, KP2D, SCORE, LABEL, ORIENT, RESIDUAL = slice(0, 4), slice(4, 12), 12, 13, 14, 15
DIMS, LOC, ROT, ALPHA, KBOX, KITTI_H, KITTI_Y, R_Y = slice(16, 19), slice(19, 22), slice(22, 25), 25, slice(26, 30), 30, 31, 32
POSE_COLS = list(range(19, 26)) + [30, 31, 32]          # what a degenerate detection turns into NaN


def wrap(a):
    """ run_network.py:312-316, 323-328: into [-pi, pi) """
    a = a % (2 * math.pi)
    if a < -math.pi:
        a += 2 * math.pi
    elif a >= math.pi:
        a -= 2 * math.pi
    return a


def pose_row(box, dims, score, label, orientation, keypoints, residual, scale, image_shape):
    """ one detection -> the 36 float64 values of its row """
    row = np.zeros(COLS)
    b = np.asarray(box, np.float64) / float(scale)                       # :114
    row[0:12] = b
    row[12:16] = float(score), float(label), float(orientation), float(residual)
    kp = np.asarray(keypoints, np.float64).reshape(4, 3)
    X_l, X_m, X_r, X_t = kp
    h, w, l = (float(v) for v in np.asarray(dims, np.float64))
    o = int(orientation)
    X_s = X_l if o in (0, 3) else X_r                                    # :147-150: outlier = 2 (X_l) for 0 and 3, 0 (X_r) for 1 and 2
    h = float(np.linalg.norm(X_t - X_m))
    l = float(np.linalg.norm(X_s - X_m))
    with np.errstate(all='ignore'):
        y_dir = (X_m - X_t) / h
        x_dir = ((X_m - X_s) if o in (0, 1) else (X_s - X_m)) / l        # :171, :226 / :182, :237
        z_dir = np.cross(x_dir, y_dir)
        location = (X_m + X_s) / 2 + (1.0 if o in (0, 2) else -1.0) * z_dir * w / 2       # :230, :186 / :175, :241
        R = np.stack([x_dir, y_dir, z_dir], axis=-1)
    row[DIMS] = h, w, l
    if not np.isfinite(R).all():                                         # a zero-length edge: no pose for this detection
        row[POSE_COLS] = np.nan
        row[KBOX] = max(b[0], 0.0), max(b[1], 0.0), min(b[2], float(image_shape[1])), min(b[3], float(image_shape[0]))
        return row
    angles = pose_np.rodrigues(R)[0][:, 0]
    row[LOC] = location
    row[ROT] = angles
    # KITTI fields, :298-330
    x_c = np.array([l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2])
    y_c = np.array([0, 0, 0, 0, -h, -h, -h, -h])
    z_c = np.array([w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2])
    X_all = pose_np.rodrigues(angles)[0].dot(np.stack([x_c, y_c, z_c], axis=0)) + location[:, None]
    r_y = wrap(angles[1])
    Y = float(X_all[1].max())
    row[KITTI_H] = Y - float(X_all[1].min())
    row[KITTI_Y] = Y
    row[R_Y] = r_y
    row[ALPHA] = wrap(r_y + math.atan2(location[2], location[0]) + 1.5 * math.pi)
    row[KBOX] = max(b[0], 0.0), max(b[1], 0.0), min(b[2], float(image_shape[1])), min(b[3], float(image_shape[0]))
    return row


def pose_rows(outputs, scales, image_shapes, score_threshold=0.05):
    """ the 8 model outputs of a batch -> (rows (B, D, 36) float64, counts (B,) int32): row d of image b belongs to detection d; a row
    whose score is not above the threshold, or whose orientation is -1, is -1 everywhere and is not counted """
    boxes, dimensions, scores, labels, orientations, keypoints, _, residuals = [np.asarray(o) for o in outputs[:8]]
    B, D = scores.shape
    rows = np.full((B, D, COLS), -1.0)
    counts = np.zeros((B,), np.int32)
    for b in range(B):
        for d in range(D):
            if not (scores[b, d] > np.float32(score_threshold)) or orientations[b, d] == -1:
                continue
            rows[b, d] = pose_row(boxes[b, d], dimensions[b, d], scores[b, d], labels[b, d], orientations[b, d], keypoints[b, d],
                                  residuals[b, d], scales[b], image_shapes[b])
            counts[b] += 1
    return rows, counts


def kitti_fields(row):
    """ the 13 numbers of a KITTI line, in its order (:329-330) """
    return (row[ALPHA], row[26], row[27], row[28], row[29], row[KITTI_H], row[17], row[18], row[19], row[KITTI_Y], row[21], row[R_Y], row[SCORE])


def kitti_lines(rows_b, count):
    """ one `%` call per row (the reference's loop) """
    return [KITTI_FORMAT % tuple(kitti_fields(r)) for r in rows_b[:count]]


def host_rows(outputs, scales, image_shapes, score_threshold=0.05):
    """ the existing host path (select_detections + recover_pose + the arithmetic of kitti_lines) laid out as rows, float64 copies of its
    float32 results: the yardstick the device rows are measured against.  Rows below the threshold stay -1. """
    from keras_retinanet_3D.utils import gpp_utils
    scores = np.asarray(outputs[2])
    B, D = scores.shape
    rows = np.full((B, D, COLS), -1.0)
    for b in range(B):
        keep = np.where(scores[b] > score_threshold)[0]
        assert np.array_equal(keep, np.arange(len(keep))), 'scores are expected in descending order'
        with np.errstate(all='ignore'):
            det = gpp_utils.recover_pose(gpp_utils.select_detections(outputs, scales[b], image_index=b, score_threshold=score_threshold))
            n = len(det['scores'])
            r = rows[b, :n]
            r[:, 0:12] = det['boxes']
            r[:, 12], r[:, 13], r[:, 14], r[:, 15] = det['scores'], det['labels'], det['orientations'], det['residuals']
            r[:, DIMS], r[:, LOC], r[:, ROT] = det['dimensions'], det['locations'], det['angles']
            X = gpp_utils.cuboid_corners(det)
            r_y = gpp_utils._wrap(det['angles'][:, 1].astype(np.float64))
            Y = X[:, 1, :].max(axis=1)
            loc = det['locations'].astype(np.float64)
            r[:, ALPHA] = gpp_utils._wrap(r_y + np.arctan2(loc[:, 2], loc[:, 0]) + 1.5 * np.pi)
            bx = det['boxes']
            r[:, 26], r[:, 27] = np.maximum(bx[:, 0], 0.0), np.maximum(bx[:, 1], 0.0)
            r[:, 28], r[:, 29] = np.minimum(bx[:, 2], image_shapes[b][1]), np.minimum(bx[:, 3], image_shapes[b][0])
            r[:, KITTI_H], r[:, KITTI_Y], r[:, R_Y] = Y - X[:, 1, :].min(axis=1), Y, r_y
            r[:, 33:36] = 0.0
    return rows


def fixture_outputs(name):
    """ the 8 outputs stored in a committed golden: a full-size fixture (frames, 100, ...) or a harness golden (in_* arrays) """
    import os
    import helpers
    g = np.load(os.path.join(helpers.GOLDEN, name))
    keys = ('boxes', 'dimensions', 'scores', 'labels', 'orientations', 'keypoints', 'keyplanes', 'residuals')
    if 'in_boxes' in g.files:
        return [g['in_' + k] for k in keys], [float(g['scale'])], [tuple(int(v) for v in g['image_shape'])]
    outs = [g[k] for k in keys]
    n = outs[0].shape[0]
    return outs, [402.0 / 375.0] * n, [(375, 1242, 3)] * n


FIXTURES = ('fullsize_resnet50_1k_f64.npz', 'fullsize_resnet50_1k_s1234t_f64.npz', 'fullsize_resnet50_1k_s2024_f64.npz',
            'harness_000007.npz', 'harness_000123.npz')

# field groups of the comparison: (name, columns, compare modulo 2 pi)
GROUPS = (('boxes', list(range(0, 12)), False), ('passed', [12, 13, 14, 15], False), ('dimensions', [16, 17, 18], False),
          ('locations', [19, 20, 21], False), ('rotation', [22, 23, 24], False), ('alpha', [25], True),
          ('kitti_box', [26, 27, 28, 29], False), ('kitti_h', [30], False), ('kitti_y', [31], False), ('r_y', [32], True))


def ulp32(x):
    """ the spacing of float32 at |x| (float64 array in, float64 out) """
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def deviation(rows, want, cols, angular):
    """ |rows - want| over the given columns (float64), modulo 2 pi for angles """
    d = np.abs(np.asarray(rows, np.float64)[..., cols] - want[..., cols])
    if angular:
        d = np.minimum(d, np.abs(d - 2 * np.pi))
    return d
