""" The oracle of KITTI's object benchmark: scalar Python, one loop per rule, Sutherland-Hodgman clipping and
the devkit's serial matching.  It shares no code with keras_retinanet_3D/utils/kitti_eval.py and none with csrc/kitti_eval.hip.

A label is a sequence of 16 numbers (type code 0 Car / 1 Van / 2 DontCare / 3 other, truncation, occlusion, alpha, box x1 y1 x2 y2,
h w l, x y z, r_y, 0); a detection is a float32 pose row of 36 numbers (include/gpp.h, gpp_pose_f32). """
import math

import numpy as np

MIN_HEIGHT = [40, 25, 25]
MAX_OCC = [0, 1, 2]
MAX_TRUNC = [0.15, 0.30, 0.50]
NAN = float('nan')


# ---------------------------------------------------------------------------------------------------- geometry
def box_corners(l, w, tx, tz, ry):
    c, s = math.cos(ry), math.sin(ry)
    out = []
    for x, z in ((l / 2.0, w / 2.0), (-l / 2.0, w / 2.0), (-l / 2.0, -w / 2.0), (l / 2.0, -w / 2.0)):
        out.append((c * x + s * z + tx, -s * x + c * z + tz))
    return out


def clip_polygon(subject, clip):
    """ Sutherland-Hodgman: the part of the convex polygon `subject` inside the counter-clockwise convex polygon `clip` """
    poly = list(subject)
    for e in range(len(clip)):
        ax, az = clip[e]
        bx, bz = clip[(e + 1) % len(clip)]
        ex, ez = bx - ax, bz - az
        out = []
        for i in range(len(poly)):
            px, pz = poly[i]
            qx, qz = poly[(i + 1) % len(poly)]
            dp = ex * (pz - az) - ez * (px - ax)
            dq = ex * (qz - az) - ez * (qx - ax)
            if dp >= 0.0:
                out.append((px, pz))
            if (dp >= 0.0) != (dq >= 0.0):
                out.append(((px * dq - qx * dp) / (dq - dp), (pz * dq - qz * dp) / (dq - dp)))
        poly = out
    return poly


def polygon_area(poly):
    if len(poly) < 3:
        return 0.0
    twice = 0.0
    for i in range(len(poly)):
        x0, z0 = poly[i]
        x1, z1 = poly[(i + 1) % len(poly)]
        twice = twice + (x0 * z1 - x1 * z0)
    return abs(twice) / 2.0


def bev_intersection(l0, w0, tx0, tz0, ry0, l1, w1, tx1, tz1, ry1):
    return polygon_area(clip_polygon(box_corners(l0, w0, tx0, tz0, ry0), box_corners(l1, w1, tx1, tz1, ry1)))


def bev_iou(l0, w0, tx0, tz0, ry0, l1, w1, tx1, tz1, ry1):
    inter = bev_intersection(l0, w0, tx0, tz0, ry0, l1, w1, tx1, tz1, ry1)
    return inter / (l0 * w0 + l1 * w1 - inter)


def image_iou(a, b, dontcare=False):
    """ a the detection's box, b the label's: x1 y1 x2 y2 """
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    if w <= 0.0 or h <= 0.0:
        return 0.0
    inter = w * h
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    if dontcare:
        return inter / area_a
    return inter / (area_a + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _div(a, b):
    """ IEEE division: a DontCare label's sides of -1 can make a union of zero (such a label is never matched in BEV or 3-D) """
    if b == 0.0:
        return NAN if (a == 0.0 or math.isnan(a)) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _any_nan(values):
    return any(math.isnan(v) for v in values)


def pair_overlaps(row, label):
    """ (image IoU, BEV IoU, 3-D IoU, image intersection over the detection's area) of one pose row and one label """
    r = [float(v) for v in row]
    g = [float(v) for v in label]
    dbox, gbox = r[26:30], g[4:8]
    if _any_nan(dbox + gbox):
        o_img = o_dc = NAN
    else:
        o_img, o_dc = image_iou(dbox, gbox), image_iou(dbox, gbox, dontcare=True)
    dh, dw, dl, dtx, dty, dtz, dry = r[30], r[17], r[18], r[19], r[31], r[21], r[32]
    gh, gw, gl, gtx, gty, gtz, gry = g[8], g[9], g[10], g[11], g[12], g[13], g[14]
    if _any_nan([dw, dl, dtx, dtz, dry, gw, gl, gtx, gtz, gry]):
        return o_img, NAN, NAN, o_dc
    inter = bev_intersection(dl, dw, dtx, dtz, dry, gl, gw, gtx, gtz, gry)
    o_bev = _div(inter, dl * dw + gl * gw - inter)
    if _any_nan([dh, dty, gh, gty]):
        return o_img, o_bev, NAN, o_dc
    hh = min(dty, gty) - max(dty - dh, gty - gh)
    hh = hh if hh > 0.0 else 0.0
    iv = inter * hh
    o_3d = _div(iv, dl * dw * dh + gl * gw * gh - iv)
    return o_img, o_bev, o_3d, o_dc


def image_overlaps(rows, labels):
    """ (4, D, A) float64; rows that are no detection (column 14 < 0) give 0 """
    rows, labels = np.asarray(rows, np.float32).reshape(-1, 36), np.asarray(labels, np.float64).reshape(-1, 16)
    out = np.zeros((4, rows.shape[0], labels.shape[0]))
    for d in range(rows.shape[0]):
        if not rows[d, 14] >= 0:
            continue
        for a in range(labels.shape[0]):
            out[:, d, a] = pair_overlaps(rows[d], labels[a])
    return out


# ---------------------------------------------------------------------------------------------------- rules
def label_status(label, difficulty):
    height = abs(label[7] - label[5])
    ignore = label[2] > MAX_OCC[difficulty] or label[1] > MAX_TRUNC[difficulty] or height < MIN_HEIGHT[difficulty]
    if label[0] == 0:
        return 1 if ignore else 0
    if label[0] == 1:
        return 1
    return -1


def detection_status(row, difficulty):
    if not row[14] >= 0:
        return -1                      # no detection at all (every detection is a Car: the devkit's "another class" never occurs)
    return 1 if abs(float(row[29]) - float(row[27])) < MIN_HEIGHT[difficulty] else 0


def match(rows, labels, overlaps, metric, difficulty, min_overlap, threshold=None):
    """ one image, one (metric, difficulty): threshold None is the devkit's compute_fp = false.
    Returns {'tp', 'fp', 'fn', 'n_gt', 'similarity', 'tp_scores': per label the true positive's score or NaN} """
    rows, labels = np.asarray(rows, np.float32).reshape(-1, 36), np.asarray(labels, np.float64).reshape(-1, 16)
    compute_fp = threshold is not None
    D, A = rows.shape[0], labels.shape[0]
    lstat = [label_status(labels[a], difficulty) for a in range(A)]
    dstat = [detection_status(rows[d], difficulty) for d in range(D)]
    out = [compute_fp and bool(rows[d, 12] < np.float32(threshold)) for d in range(D)]
    assigned = [False] * D
    tp = fp = fn = 0
    similarity = 0.0
    tp_scores = [NAN] * A
    for a in range(A):
        if lstat[a] == -1:
            continue
        cand, cand_ignored, max_ov, best = -1, False, 0.0, -math.inf
        for d in range(D):
            if dstat[d] == -1 or assigned[d] or out[d]:
                continue
            o = overlaps[metric, d, a]
            if not compute_fp and o > min_overlap and rows[d, 12] > best:
                cand, best = d, rows[d, 12]
            elif compute_fp and o > min_overlap and (o > max_ov or cand_ignored) and dstat[d] == 0:
                max_ov, cand, cand_ignored = o, d, False
            elif compute_fp and o > min_overlap and cand == -1 and dstat[d] == 1:
                cand, cand_ignored = d, True
        if cand == -1 and lstat[a] == 0:
            fn += 1
        elif cand != -1 and (lstat[a] == 1 or dstat[cand] == 1):
            assigned[cand] = True
        elif cand != -1:
            tp += 1
            tp_scores[a] = rows[cand, 12]
            if metric == 0 and compute_fp:
                similarity = similarity + (1.0 + math.cos(float(labels[a, 3]) - float(rows[cand, 25]))) / 2.0
            assigned[cand] = True
    if compute_fp:
        for d in range(D):
            if not (assigned[d] or dstat[d] == -1 or dstat[d] == 1 or out[d]):
                fp += 1
        if metric == 0:
            stuff = 0
            for a in range(A):
                if labels[a, 0] != 2:
                    continue
                for d in range(D):
                    if assigned[d] or dstat[d] == -1 or dstat[d] == 1 or out[d]:
                        continue
                    if overlaps[3, d, a] > min_overlap:
                        assigned[d] = True
                        stuff += 1
            fp -= stuff
    return {'tp': tp, 'fp': fp, 'fn': fn, 'n_gt': sum(1 for s in lstat if s == 0), 'similarity': similarity,
            'tp_scores': np.array(tp_scores, np.float32)}


def thresholds(scores, n_gt):
    v = sorted((np.float32(s) for s in scores), reverse=True)
    out, cur = [], 0.0
    for i in range(len(v)):
        l = (i + 1) / float(n_gt)
        r = (i + 2) / float(n_gt) if i < len(v) - 1 else l
        if (r - cur) < (cur - l) and i < len(v) - 1:
            continue
        out.append(v[i])
        cur += 1.0 / 40.0
        if len(out) == 41:
            break
    return out


def evaluate(rows_list, labels_list, min_overlap=(0.7, 0.7, 0.7)):
    """ the dataset level: {(metric index, difficulty index): {'ap_r40', 'ap_r11', 'aos_r40', 'aos_r11', 'thresholds', 'tp', 'fp', 'fn'}} """
    overlaps = [image_overlaps(r, g) for r, g in zip(rows_list, labels_list)]
    result = {}
    for m in range(3):
        for d in range(3):
            v, n_gt = [], 0
            for r, g, o in zip(rows_list, labels_list, overlaps):
                one = match(r, g, o, m, d, min_overlap[m])
                v += [s for s in one['tp_scores'] if not math.isnan(s)]
                n_gt += one['n_gt']
            thr = thresholds(v, n_gt) if n_gt else []
            precision, aos = [0.0] * 41, [0.0] * 41
            tps, fps, fns = [], [], []
            for k, t in enumerate(thr):
                tp = fp = fn = 0
                sim = 0.0
                for r, g, o in zip(rows_list, labels_list, overlaps):
                    one = match(r, g, o, m, d, min_overlap[m], t)
                    tp, fp, fn, sim = tp + one['tp'], fp + one['fp'], fn + one['fn'], sim + one['similarity']
                tps.append(tp), fps.append(fp), fns.append(fn)
                if tp + fp > 0:
                    precision[k], aos[k] = tp / float(tp + fp), sim / float(tp + fp)
            for k in range(39, -1, -1):
                precision[k], aos[k] = max(precision[k], precision[k + 1]), max(aos[k], aos[k + 1])
            result[(m, d)] = {'ap_r40': 100.0 * sum(precision[1:]) / 40.0, 'ap_r11': 100.0 * sum(precision[0::4]) / 11.0,
                              'aos_r40': 100.0 * sum(aos[1:]) / 40.0, 'aos_r11': 100.0 * sum(aos[0::4]) / 11.0,
                              'thresholds': [float(t) for t in thr], 'tp': tps, 'fp': fps, 'fn': fns}
    return result


# ---------------------------------------------------------------------------------------------------- builders for the tests
def make_label(kind=0, box=(100.0, 100.0, 200.0, 160.0), hwl=(1.5, 1.75, 4.0), xyz=(2.0, 1.5, 20.0), ry=0.0, alpha=0.0, trunc=0.0, occ=0):
    return [float(kind), float(trunc), float(occ), float(alpha)] + [float(v) for v in box] + [float(v) for v in hwl] + \
           [float(v) for v in xyz] + [float(ry), 0.0]


def make_row(score, box=(100.0, 100.0, 200.0, 160.0), hwl=(1.5, 1.75, 4.0), xyz=(2.0, 1.5, 20.0), ry=0.0, alpha=0.0):
    row = np.zeros(36, np.float32)
    row[12], row[25], row[26:30] = score, alpha, box
    row[30], row[17], row[18] = hwl
    row[19], row[31], row[21] = xyz
    row[32] = ry
    return row


def padding_row():
    return np.full(36, -1.0, np.float32)


def row_like(label, score, **changes):
    """ the detection that reproduces a label exactly, with changes """
    kw = {'box': label[4:8], 'hwl': label[8:11], 'xyz': label[11:14], 'ry': label[14], 'alpha': label[3]}
    kw.update(changes)
    return make_row(score, **kw)


def random_scene(rng, n_labels, n_dets, near=True):
    """ labels around the origin of a 40 m stretch, detections jittered around some of them (centres within +-3 m) """
    labels, rows = [], []
    for _ in range(n_labels):
        l, w, h = rng.uniform(3, 5), rng.uniform(1.5, 2), rng.uniform(1.4, 1.8)
        x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
        labels.append(make_label(kind=int(rng.choice([0, 0, 0, 1, 2, 3])), box=(x1, y1, x1 + rng.uniform(30, 200), y1 + rng.uniform(20, 120)),
                                 hwl=(h, w, l), xyz=(rng.uniform(-20, 20), rng.uniform(1, 2), rng.uniform(5, 60)), ry=rng.uniform(-math.pi, math.pi),
                                 alpha=rng.uniform(-math.pi, math.pi), trunc=float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6])), occ=int(rng.integers(0, 4))))
    for _ in range(n_dets):
        g = labels[int(rng.integers(0, n_labels))]
        tight = rng.random() < 0.6
        j = 0.15 if tight else 3.0
        box = [g[4] + rng.uniform(-1, 1) * (3 if tight else 40), g[5] + rng.uniform(-1, 1) * (2 if tight else 30),
               g[6] + rng.uniform(-1, 1) * (3 if tight else 40), g[7] + rng.uniform(-1, 1) * (2 if tight else 30)]
        rows.append(make_row(rng.uniform(0.05, 1.0), box=box,
                             hwl=(g[8] * rng.uniform(0.95, 1.05), g[9] * rng.uniform(0.95, 1.05), g[10] * rng.uniform(0.95, 1.05)),
                             xyz=(g[11] + rng.uniform(-j, j), g[12] + rng.uniform(-0.1, 0.1), g[13] + rng.uniform(-j, j)),
                             ry=g[14] + (rng.uniform(-0.05, 0.05) if tight else rng.uniform(-math.pi, math.pi)), alpha=g[3] + rng.uniform(-0.3, 0.3)))
    return np.array(rows, np.float32).reshape(-1, 36), np.array(labels, np.float64).reshape(-1, 16)


def write_dataset(tmp_path, n=3, seed=23):
    """ n images: label files (15 fields) and the result files kitti_lines_from_rows writes for jittered detections """
    from keras_retinanet_3D.utils.gpp_utils import kitti_lines_from_rows          # (the writer of the project's result files)
    rng = np.random.default_rng(seed)
    label_dir, result_dir = tmp_path / 'label_2', tmp_path / 'results'
    label_dir.mkdir(), result_dir.mkdir()
    names = {0: 'Car', 1: 'Van', 2: 'DontCare', 3: 'Cyclist'}
    for i in range(n):
        rows, labels = random_scene(rng, 6, 12)
        with open(label_dir / '{:06d}.txt'.format(i), 'w') as f:
            for g in labels:
                f.write('{} {:.2f} {:d} '.format(names[int(g[0])], g[1], int(g[2])) + ' '.join('{:.2f}'.format(v) for v in g[3:15]) + '\n')
        full = np.zeros((12, 36), np.float32)
        full[:, :] = rows
        with open(result_dir / '{:06d}.txt'.format(i), 'w') as f:
            f.write(kitti_lines_from_rows(full, 12))
    return str(label_dir), str(result_dir)
