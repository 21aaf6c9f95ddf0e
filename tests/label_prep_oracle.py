""" ORACLE (test infrastructure): the reference's MATLAB label preparation -- label_prep/create_mod_labels.m, computeBox3D.m and
projectToImage.m -- restated object by object and corner by corner in scalar Python, independent of utils/label_prep.py.  Matrix
products are written out as MATLAB's row-times-column sums (zero terms included), every value a Python float (IEEE double).

cos and sin are NumPy's, as in the product: MATLAB's own last bit is the part that is unpinned. """
import math
import os

import numpy as np

FACE_X = (1, 1, -1, -1, 1, 1, -1, -1)          # computeBox3D.m:22-24: x = +-l/2, y = 0 or -h, z = +-w/2
FACE_Y = (0, 0, 0, 0, -1, -1, -1, -1)
FACE_Z = (1, -1, -1, 1, 1, -1, -1, 1)
# create_mod_labels.m:57-100, corner numbers as written there (1-based): x_l, x_m, x_r, x_t
TABLE = {0: (3, 2, 1, 6), 1: (2, 1, 4, 5), 2: (4, 3, 2, 7), 3: (1, 4, 3, 8)}


def compute_box_3d(h, w, l, t, ry, P):
    """ computeBox3D.m: the (2, 8) projected corners as two lists, or None when a corner lies behind Z = 0.1 """
    c, s = float(np.cos(np.float64(ry))), float(np.sin(np.float64(ry)))
    R = ((c, 0.0, s), (0.0, 1.0, 0.0), (-s, 0.0, c))
    corners = []
    for k in range(8):
        x = l / 2 if FACE_X[k] > 0 else -l / 2
        y = 0.0 if FACE_Y[k] == 0 else -h
        z = w / 2 if FACE_Z[k] > 0 else -w / 2
        p = [(R[r][0] * x + R[r][1] * y) + R[r][2] * z for r in range(3)]
        corners.append((p[0] + t[0], p[1] + t[1], p[2] + t[2]))
    if any(p[2] < 0.1 for p in corners):
        return None
    us, vs = [], []
    for X, Y, Z in corners:                      # projectToImage.m
        q = [((P[r][0] * X + P[r][1] * Y) + P[r][2] * Z) + P[r][3] * 1.0 for r in range(3)]
        us.append(q[0] / q[2])
        vs.append(q[1] / q[2])
    return us, vs


def mod_row(label, P):
    """ one (16,) label row (type code, truncation, occlusion, alpha, box, h w l, x y z, r_y, 0) -> the 20 values of its mod line.
    Raises ValueError where the script's if / elseif chain would fall through. """
    label = [float(v) for v in label]
    P = [[float(v) for v in row] for row in np.asarray(P).reshape(3, 4)]
    kind, trunc, occ, alpha = label[0:4]
    h, w, l = label[8:11]
    proj = compute_box_3d(h, w, l, label[11:14], label[14], P)
    if proj is None:
        return [2.0, -1.0, -1.0, -10.0] + label[4:8] + [-10000.0] * 8 + [h, w, l, -1.0]
    deg = (180.0 / math.pi) * alpha              # rad2deg
    if 0 <= deg < 90:
        cls = 0
    elif 90 <= deg < 180:
        cls = 1
    elif -90 <= deg < 0:
        cls = 2
    elif -180 <= deg < -90:
        cls = 3
    else:
        raise ValueError('alpha {} is outside [-180, 180) degrees'.format(alpha))
    us, vs = proj
    kp = []
    for corner in TABLE[cls]:
        kp += [us[corner - 1], vs[corner - 1]]
    return [kind, trunc, occ, alpha, min(us), min(vs), max(us), max(vs)] + kp + [h, w, l, float(cls)]


def mod_rows(labels, P):
    labels = np.asarray(labels, np.float64).reshape(-1, 16)
    return np.array([mod_row(g, P) for g in labels], np.float64).reshape(-1, 20)


def make_label(kind=0, trunc=0.0, occ=0, alpha=0.0, box=(0.0, 0.0, 0.0, 0.0), hwl=(1.5, 1.6, 4.0), xyz=(0.0, 1.6, 20.0), ry=0.0):
    return np.array([kind, trunc, occ, alpha] + list(box) + list(hwl) + list(xyz) + [ry, 0.0], np.float64)


def dont_care(box=(503.0, 169.0, 590.0, 190.0)):
    """ a DontCare line of label_2 """
    return make_label(kind=2, trunc=-1.0, occ=-1, alpha=-10.0, box=box, hwl=(-1.0, -1.0, -1.0), xyz=(-1000.0, -1000.0, -1000.0), ry=-10.0)


def seeded_scene(seed, n, P_offset=True, z_range=(6.0, 70.0), kinds=(0, 0, 0, 1, 3), behind=0.1):
    """ n KITTI-like objects: alpha = r_y - atan2(x, z) wrapped into [-pi, pi), about `behind` of them moved behind the camera.
    Returns (labels (n, 16), P (3, 4)). """
    rng = np.random.default_rng(seed)
    P = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    if not P_offset:
        P[:, 3] = 0.0
    out = []
    for _ in range(n):
        z = rng.uniform(*z_range)
        x = rng.uniform(-0.45, 0.45) * z
        ry = rng.uniform(-math.pi, math.pi)
        alpha = (ry - math.atan2(x, z) + math.pi) % (2 * math.pi) - math.pi
        if rng.random() < behind:
            z = rng.uniform(-5.0, 2.0)
        x1, y1 = rng.uniform(0, 1100), rng.uniform(120, 250)
        out.append(make_label(kind=int(rng.choice(kinds)), trunc=float(rng.choice([0.0, 0.1, 0.4])), occ=int(rng.integers(0, 4)), alpha=alpha,
                              box=(x1, y1, x1 + rng.uniform(30, 140), y1 + rng.uniform(20, 110)),
                              hwl=(rng.uniform(1.4, 1.8), rng.uniform(1.5, 1.8), rng.uniform(3.5, 4.8)),
                              xyz=(x, rng.uniform(1.4, 1.9), z), ry=ry))
    return np.array(out, np.float64).reshape(-1, 16), P


def write_dataset(root, scenes):
    """ label_2 / calib directories of `scenes` = [(names, labels (n, 16), P)], values with the decimals of a KITTI file """
    label_dir, calib_dir = os.path.join(str(root), 'label_2'), os.path.join(str(root), 'calib')
    os.makedirs(label_dir), os.makedirs(calib_dir)
    for i, (names, labels, P) in enumerate(scenes):
        with open(os.path.join(label_dir, '%06d.txt' % i), 'w') as f:
            for name, g in zip(names, labels):
                f.write('{} {:.2f} {:d} '.format(name, g[1], int(g[2])) + ' '.join('%.2f' % v for v in g[3:15]) + '\n')
        with open(os.path.join(calib_dir, '%06d.txt' % i), 'w') as f:
            for cam in range(4):
                f.write('P{}: '.format(cam) + ' '.join('%.12e' % v for v in (P if cam == 2 else P * (cam + 2.0)).ravel()) + '\n')
            f.write('R0_rect: ' + ' '.join(['1.0'] * 9) + '\n')
    return label_dir, calib_dir


NAMES = {0: 'Car', 1: 'Van', 2: 'DontCare', 3: 'Cyclist'}


def three_scenes():
    scenes = []
    for seed, n in ((11, 7), (12, 0), (13, 5)):
        labels, P = seeded_scene(seed, n, kinds=(0, 0, 1, 3))
        if n:
            labels[n - 1] = dont_care()
        scenes.append(([NAMES[int(k)] for k in labels[:, 0]], labels, P))
    return scenes
