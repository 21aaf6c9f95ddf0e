"""
KITTI keypoint ("mod") labels from a stock KITTI download, and the accuracy ceiling of ground-plane polling on them -- DESIGN.md section
4.18 is the specification, a restatement of the reference's MATLAB scripts label_prep/create_mod_labels.m, computeBox3D.m and
projectToImage.m.  Parity with MATLAB itself is UNPINNED (no MATLAB at hand; its cos / sin may round the last bit differently); what is
pinned is the round trip labels -> keypoints -> polling -> pose -> labels (tests/test_label_prep_cpu.py) through stages that are pinned
to the reference's Python.

Two forms of one computation:
    prepare            NumPy, no GPU and no library: elementwise float64, every operation separate (no BLAS: nothing contracts)
    prepare_device     csrc/label_prep.hip (gpp_label_prep_f64), one thread per (image, label row)
Both take cos(r_y) and sin(r_y) from np.cos / np.sin on the host, so that the two results are equal bit for bit.

polling_ceiling runs ground-truth keypoints through the product's own kernels -- gpp_label_prep_f64 -> gpp_poll_f32 -> gpp_pose_f32 ->
gpp_kitti_overlaps_f64 / gpp_kitti_stats_f64 -- and so measures what the plane database and the polling cost in AP given perfect 2-D
keypoints.  It is device-only, like every other caller of the polling kernel.

A label is a (16,) float64 row as utils/kitti_eval.read_label_file gives it; a mod row is (20,) float64:
    0 type code | 1-3 truncation occlusion alpha | 4-7 box | 8-15 xl yl xm ym xr yr xt yt | 16-18 h w l | 19 orientation class
"""
import os

import numpy as np

from . import kitti_eval
from .kitti_eval import LABEL_COLS

MOD_COLS = 20
DEG_PER_RAD = 180.0 / np.pi                                 # MATLAB's rad2deg: (180 / pi) * alpha
MIN_Z = 0.1                                                 # computeBox3D.m:33
DEFAULT_IMAGE_SIZE = (376, 1242)                            # KITTI's largest frame: clips no label box
CAR = 1 << kitti_eval.TYPE_CODES['Car']                     # det_types masks: bit `type code`
VAN = 1 << kitti_eval.TYPE_CODES['Van']
# keypoint (l, m, r, t) -> corner (0-based) per orientation class, create_mod_labels.m:57-100 (utils/synthetic.KEYPOINT_CORNERS, 1-based)
_CORNERS = ((2, 1, 0, 5), (1, 0, 3, 4), (3, 2, 1, 6), (0, 3, 2, 7))
MOD_FORMAT = '%s %f %d %f' + ' %f' * 15 + ' %d\n'            # create_mod_labels.m:108


# ---------------------------------------------------------------------------------------------------- files
def read_labels(path):
    """ a label_2 file -> (type names, (n, 16) float64 rows as kitti_eval.read_label_file gives them) """
    names = []
    rows = kitti_eval._read_lines(path, 'label', names)
    rows[:, 15] = 0.0
    return names, rows


def read_calibration(path):
    """ the camera-2 matrix (3, 4) float64 of a KITTI calibration file: the line that starts with 'P2:' (the third) """
    with open(path, 'r') as f:
        lines = f.readlines()
    line = ([v for v in lines if v.startswith('P2:')] or lines[2:3] or [''])[0]
    values = line.split(':', 1)[-1].split()
    if len(values) != 12:
        raise ValueError('{}: no P2 line with 12 numbers'.format(path))
    return np.array([float(v) for v in values], np.float64).reshape(3, 4)


def format_lines(names, mod):
    """ the text of a mod label file: MATLAB's '%s %f %d %f ... %f %d\\n' per row; a demoted row is written as DontCare """
    mod = np.asarray(mod, np.float64).reshape(-1, MOD_COLS)
    if len(names) != mod.shape[0]:
        raise ValueError('{} names for {} rows'.format(len(names), mod.shape[0]))
    out = []
    for name, r in zip(names, mod):
        demoted = r[19] == -1.0
        out.append(MOD_FORMAT % (('DontCare' if demoted else name, r[1], int(r[2])) + tuple(r[3:19].tolist()) + (int(r[19]),)))
    return ''.join(out)


# ---------------------------------------------------------------------------------------------------- the host form
def trig_of(labels):
    """ (..., 16) labels -> (..., 2) float64: cos(r_y), sin(r_y).  The one place either form takes them from. """
    ry = np.asarray(labels, np.float64)[..., 14]
    return np.stack([np.cos(ry), np.sin(ry)], axis=-1)


def _lower(a, b):
    return np.where(b < a, b, a)


def _upper(a, b):
    return np.where(b > a, b, a)


def prepare_rows(labels, P, trig=None, strict=True):
    """ labels (..., 16), P (..., 3, 4) broadcast against them, trig (..., 2) -> (mod (..., 20), valid (...) bool).  Every step an
    elementwise float64 operation in the order of csrc/label_prep.hip.  strict: a row in front of the camera whose alpha lies outside
    [-180, 180) degrees raises ValueError (the MATLAB script would reuse the previous object's variables); otherwise it is demoted,
    as the kernel does. """
    g = np.asarray(labels, np.float64)
    if g.shape[-1] != LABEL_COLS:
        raise ValueError('labels must be (..., {}), got {}'.format(LABEL_COLS, g.shape))
    lead = g.shape[:-1]
    P = np.broadcast_to(np.asarray(P, np.float64), lead + (3, 4))
    t = trig_of(g) if trig is None else np.asarray(trig, np.float64)
    c, s = t[..., 0], t[..., 1]
    ns = -s
    h, w, l, tx, ty, tz = (g[..., k] for k in range(8, 14))
    hl, hw = l / 2.0, w / 2.0
    mod = np.empty(lead + (MOD_COLS,), np.float64)
    with np.errstate(all='ignore'):
        # computeBox3D.m:22-30: the four (x, z) of the bottom face, the same four at y = -h
        xs, zs = (hl, hl, -hl, -hl), (hw, -hw, -hw, hw)
        X = [(c * x + s * z) + tx for x, z in zip(xs, zs)]
        Z = [(ns * x + c * z) + tz for x, z in zip(xs, zs)]
        Y = (0.0 + ty, (-h) + ty)
        behind = (Z[0] < MIN_Z) | (Z[1] < MIN_Z) | (Z[2] < MIN_Z) | (Z[3] < MIN_Z)
        deg = DEG_PER_RAD * g[..., 3]
        o = np.full(lead, -1, np.int64)
        o[(deg >= 0.0) & (deg < 90.0)] = 0
        o[(deg >= 90.0) & (deg < 180.0)] = 1
        o[(deg >= -90.0) & (deg < 0.0)] = 2
        o[(deg >= -180.0) & (deg < -90.0)] = 3
        if strict and (~behind & (o < 0)).any():
            raise ValueError('alpha outside [-180, 180) degrees in {} row(s): {}'.format(
                int((~behind & (o < 0)).sum()), g[..., 3][~behind & (o < 0)][:4].tolist()))
        valid = ~behind & (o >= 0)
        # projectToImage.m: ((P_r0 X + P_r1 Y) + P_r2 Z) + P_r3, then the two divisions; corners 1-4 bottom, 5-8 top
        px, py = [], []
        for k in range(8):
            Xk, Yk, Zk = X[k & 3], Y[k >> 2], Z[k & 3]
            u, v, d = (((P[..., r, 0] * Xk + P[..., r, 1] * Yk) + P[..., r, 2] * Zk) + P[..., r, 3] for r in range(3))
            px.append(u / d)
            py.append(v / d)
        x1, y1, x2, y2 = px[0], py[0], px[0], py[0]
        for k in range(1, 8):
            x1, y1, x2, y2 = _lower(x1, px[k]), _lower(y1, py[k]), _upper(x2, px[k]), _upper(y2, py[k])
        mod[..., 0:4] = g[..., 0:4]
        for k, v in enumerate((x1, y1, x2, y2)):
            mod[..., 4 + k] = v
        for j in range(4):                                    # keypoint l m r t: o == 0 ? . : (o == 1 ? . : (o == 2 ? . : .))
            kx, ky = px[_CORNERS[3][j]], py[_CORNERS[3][j]]
            for cls in (2, 1, 0):
                kx, ky = np.where(o == cls, px[_CORNERS[cls][j]], kx), np.where(o == cls, py[_CORNERS[cls][j]], ky)
            mod[..., 8 + 2 * j], mod[..., 9 + 2 * j] = kx, ky
        mod[..., 16:19] = g[..., 8:11]
        mod[..., 19] = o
    # create_mod_labels.m:37-55
    demoted = np.full(MOD_COLS, -10000.0)
    demoted[0:4], demoted[19] = (2.0, -1.0, -1.0, -10.0), -1.0
    keep = np.zeros(MOD_COLS, bool)
    keep[4:8], keep[16:19] = True, True
    own = np.concatenate([g[..., 0:4], g[..., 4:8], np.zeros(lead + (8,)), g[..., 8:11], np.zeros(lead + (1,))], axis=-1)
    mod = np.where(valid[..., None], mod, np.where(keep, own, demoted))
    return mod, valid


def prepare(labels, P, strict=True):
    """ the host form for one image: labels (n, 16), P (3, 4) -> mod (n, 20) float64 """
    labels = np.asarray(labels, np.float64).reshape(-1, LABEL_COLS)
    return prepare_rows(labels, np.asarray(P, np.float64).reshape(3, 4), strict=strict)[0]


def prepare_batch(labels, label_counts, P, trig=None, det_types=0, own_box=True):
    """ the host form of one gpp_label_prep_f64 launch: labels (B, A, 16), label_counts (B,), P (B, 3, 4) ->
    (mod (B, A, 20), (boxes (B, A, 12), dims (B, A, 3), scores (B, A) float32, labels (B, A), orientations (B, A) int32)).  Rows at or
    beyond the count are -1; an out-of-range alpha demotes the row. """
    labels = np.asarray(labels, np.float64)
    B, A = labels.shape[:2]
    P = np.asarray(P, np.float64).reshape(B, 1, 3, 4)
    mod, valid = prepare_rows(labels, P, trig, strict=False)
    live = np.arange(A)[None, :] < np.clip(np.asarray(label_counts).reshape(B, 1), 0, A)
    mod = np.where(live[..., None], mod, -1.0)
    valid = valid & live
    kind = labels[..., 0]
    with np.errstate(invalid='ignore'):
        inside = valid & (kind >= 0.0) & (kind < 32.0)
    code = np.where(inside, kind, 0.0).astype(np.int64)
    det = inside & (((int(det_types) & 0xffffffff) >> code) & 1).astype(bool)
    box = labels[..., 4:8] if own_box else mod[..., 4:8]
    boxes = np.where(det[..., None], np.concatenate([box, mod[..., 8:16]], axis=-1), -1.0).astype(np.float32)
    dims = np.where(det[..., None], mod[..., 16:19], -1.0).astype(np.float32)
    scores = np.where(det, 1.0, -1.0).astype(np.float32)
    det_labels = np.where(det, 0, -1).astype(np.int32)
    orient = np.where(det, mod[..., 19], -1.0).astype(np.int32)
    return mod, (boxes, dims, scores, det_labels, orient)


# ---------------------------------------------------------------------------------------------------- the device form
def _upload(labels_list, P_list, A=None, device=None):
    import torch
    from ..backend import hip
    dev = hip.require_device() if device is None else device
    packed, counts = kitti_eval.pack_labels(labels_list, A)
    P = np.ascontiguousarray(np.asarray(P_list, np.float64).reshape(len(labels_list), 3, 4))
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev, non_blocking=True)  # noqa: E731
    return up(packed), up(counts), up(P), up(trig_of(packed))


def prepare_device(labels_list, P_list, det_types=0, own_box=True, detections=False):
    """ the device form for a batch of images: per image the (n_b, 16) labels and the (3, 4) matrix -> per image the (n_b, 20) mod rows
    (NumPy); with `detections` also the five (B, A, ...) arrays of the decode's layout (NumPy).  One upload, one launch. """
    from ..backend import hip
    if len(labels_list) != len(P_list):
        raise ValueError('{} label arrays and {} matrices'.format(len(labels_list), len(P_list)))
    if not labels_list:
        return ([], None) if detections else []
    labels_d, counts_d, P_d, trig_d = _upload(labels_list, P_list)
    mod_d, det_d = hip.label_prep(labels_d, counts_d, P_d, trig_d, det_types, own_box, detections)
    mod, counts = mod_d.cpu().numpy(), counts_d.cpu().numpy()
    out = [mod[b, :counts[b]].copy() for b in range(len(labels_list))]
    if detections:
        return out, tuple(t.cpu().numpy() for t in det_d)
    return out


WRITE_CHUNK = 4096                                          # images per launch of write_mod_labels(device=True)


def write_mod_labels(label_dir, calib_dir, out_dir, device=False):
    """ a mod label file in `out_dir` for every label_2 file of `label_dir` (sorted by name), with the calibration file of the same name.
    device=False: NumPy; device=True: csrc/label_prep.hip, WRITE_CHUNK images per launch -- the same bytes.  Returns the file count. """
    files = sorted(f for f in os.listdir(label_dir) if f.endswith('.txt'))
    os.makedirs(out_dir, exist_ok=True)
    for at in range(0, len(files), WRITE_CHUNK):
        part = files[at:at + WRITE_CHUNK]
        read = [read_labels(os.path.join(label_dir, f)) for f in part]
        Ps = [read_calibration(os.path.join(calib_dir, f)) for f in part]
        for f, (_, rows), P in zip(part, read, Ps):           # the contract, in both forms: an out-of-range alpha raises before anything runs
            try:
                _check_alpha(rows, P)
            except ValueError as e:
                raise ValueError('{}: {}'.format(os.path.join(label_dir, f), e))
        mods = prepare_device([r for _, r in read], Ps) if device else [prepare(r, P) for (_, r), P in zip(read, Ps)]
        for f, (names, _), mod in zip(part, read, mods):
            with open(os.path.join(out_dir, f), 'w') as out:
                out.write(format_lines(names, mod))
    return len(files)


def _check_alpha(rows, P):
    """ the strict rule without the projection: only the corner depths and the angle (the device form's host-side contract check) """
    rows = np.asarray(rows, np.float64).reshape(-1, LABEL_COLS)
    deg = DEG_PER_RAD * rows[:, 3]
    with np.errstate(invalid='ignore'):
        bad = ~((deg >= -180.0) & (deg < 180.0))
    if bad.any():
        prepare_rows(rows[bad], P, strict=True)


# ---------------------------------------------------------------------------------------------------- the ceiling of polling
def _wrap(a):
    a = np.mod(a + np.pi, 2.0 * np.pi) - np.pi
    return a


def _load_planes(planes):
    if isinstance(planes, (str, bytes, os.PathLike)):
        import scipy.io
        planes = scipy.io.loadmat(planes)['road_planes_database']
    planes = np.ascontiguousarray(np.asarray(planes, np.float32).reshape(-1, 4))
    if planes.shape[0] < 1:
        raise ValueError('the plane database is empty')
    return planes


def error_summary(rows_list, labels_list):
    """ the rows of polling_ceiling against the labels they were made from (row a of an image belongs to label a): over the rows that are
    detections the median / max distance of the location (columns 19, 31, 21 against x y z), of r_y (column 32, wrapped), and the share
    of rows with a NaN pose """
    loc, ang, n, nan = [], [], 0, 0
    for r, g in zip(rows_list, labels_list):
        r, g = np.asarray(r, np.float64).reshape(-1, kitti_eval.POSE_COLS), np.asarray(g, np.float64).reshape(-1, LABEL_COLS)
        det = r[:g.shape[0], 14] >= 0.0
        r, g = r[:g.shape[0]][det], g[det]
        bad = np.isnan(r[:, [19, 31, 21, 32]]).any(axis=1)
        n, nan = n + r.shape[0], nan + int(bad.sum())
        r, g = r[~bad], g[~bad]
        loc.append(np.sqrt((r[:, 19] - g[:, 11]) ** 2 + (r[:, 31] - g[:, 12]) ** 2 + (r[:, 21] - g[:, 13]) ** 2))
        ang.append(np.abs(_wrap(r[:, 32] - g[:, 14])))
    loc, ang = np.concatenate(loc + [np.zeros(0)]), np.concatenate(ang + [np.zeros(0)])
    stat = lambda v, f: float(f(v)) if v.size else float('nan')  # noqa: E731
    return {'detections': n, 'nan_share': (nan / n) if n else 0.0,
            'location_error_median_m': stat(loc, np.median), 'location_error_max_m': stat(loc, np.max),
            'r_y_error_median_rad': stat(ang, np.median), 'r_y_error_max_rad': stat(ang, np.max)}


def ceiling_chunk(labels_list, P_list, planes_d, sizes, det_types=CAR, A=None):
    """ one chunk of polling_ceiling, launched on the current stream and not waited for: labels, trig, P and pinv(P) go up once, then
    gpp_label_prep_f64 (own_box = 1) -> gpp_poll_f32 -> gpp_pose_f32 (scale 1) -> gpp_kitti_overlaps_f64, everything in place.
    Returns the kitti_eval.DeviceChunk (its rows are the pose rows, D = A). """
    import torch
    from ..backend import hip
    from . import gpp_utils
    dev = planes_d.device
    labels_d, counts_d, P_d, trig_d = _upload(labels_list, P_list, A, dev)
    B = len(labels_list)
    pinv = np.stack([np.linalg.pinv(np.asarray(P, np.float64).reshape(3, 4)) for P in P_list]).astype(np.float32)
    pinv_d = torch.as_tensor(pinv).to(dev, non_blocking=True)
    info = np.empty((B, 3), np.float32)
    info[:, 0], info[:, 1:] = 1.0, np.asarray(sizes, np.float64).reshape(B, 2)
    info_d = torch.as_tensor(info).to(dev, non_blocking=True)
    _, det = hip.label_prep(labels_d, counts_d, P_d, trig_d, det_types, True, True)
    boxes, dims, scores, det_labels, orient = det
    keypoints, _, residuals = gpp_utils.fit_road_planes(boxes, dims, orient, pinv_d, planes_d)
    rows = torch.empty((B, int(labels_d.shape[1]), hip.GPP_POSE_COLS), dtype=torch.float32, device=dev)
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    hip.check(hip.lib().gpp_pose_f32(hip.ptr(boxes), hip.ptr(dims), hip.ptr(scores), hip.ptr(det_labels), hip.ptr(orient), hip.ptr(keypoints),
                                     hip.ptr(residuals), hip.ptr(info_d), B, int(rows.shape[1]), gpp_utils.POSE_SCORE_THRESHOLD,
                                     hip.ptr(rows), hip.ptr(counts), hip.stream_ptr()), 'gpp_pose_f32')
    return kitti_eval.DeviceChunk(rows, labels_d, counts_d, hip.kitti_overlaps(rows, labels_d, counts_d))


def polling_ceiling(label_dir, calib_dir, planes, *, min_overlap=(0.7, 0.7, 0.7), image_sizes=None, return_rows=False, chunk_images=None):
    """ KITTI's Car benchmark of ground-plane polling fed with PERFECT 2-D keypoints: the label_2 files of `label_dir` (sorted by name)
    and the calibration files of the same names in `calib_dir` are prepared, polled against `planes` ((N, 4), or the path of a .mat
    database), turned into poses and scored against themselves, all on the device; the dataset is cut into chunks as
    kitti_eval.chunk_images does (`chunk_images` overrides the number of images per chunk).
    image_sizes: per image (height, width) -- a sequence in file order or a dict keyed by the file's stem -- for the clipping of the
    boxes; by default 376 x 1242, KITTI's largest frame, which clips no label box.
    Returns evaluate_kitti's dict plus 'summary' (error_summary of the rows against the labels, host-computed) and, with return_rows,
    'rows': per image the (n_b, 36) float32 pose rows.  Raises GppError without a GPU. """
    import torch
    from ..backend import hip
    dev = hip.require_device()
    min_overlap = kitti_eval._check_min_overlap(min_overlap)
    planes_d = torch.as_tensor(_load_planes(planes)).to(dev)
    files = sorted(f for f in os.listdir(label_dir) if f.endswith('.txt'))
    labels_list = [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in files]
    P_list = [read_calibration(os.path.join(calib_dir, f)) for f in files]
    for f, g, P in zip(files, labels_list, P_list):
        try:
            _check_alpha(g, P)
        except ValueError as e:
            raise ValueError('{}: {}'.format(os.path.join(label_dir, f), e))
    if image_sizes is None:
        sizes = [DEFAULT_IMAGE_SIZE] * len(files)
    elif isinstance(image_sizes, dict):
        sizes = [tuple(image_sizes.get(os.path.splitext(f)[0], DEFAULT_IMAGE_SIZE))[:2] for f in files]
    else:
        sizes = [tuple(s)[:2] for s in image_sizes]
        if len(sizes) != len(files):
            raise ValueError('{} image sizes for {} label files'.format(len(sizes), len(files)))
    A = max([g.shape[0] for g in labels_list] + [1])
    if A > kitti_eval.MAX_LABELS:
        raise ValueError('the device form takes up to {} labels per image, got {}'.format(kitti_eval.MAX_LABELS, A))
    step = kitti_eval.chunk_images(A, A) if chunk_images is None else max(1, int(chunk_images))
    chunks = [ceiling_chunk(labels_list[at:at + step], P_list[at:at + step], planes_d, sizes[at:at + step], CAR, A)
              for at in range(0, len(files), step)]
    result = kitti_eval.evaluate_chunks(chunks, min_overlap)
    # the summary reads the location, r_y and orientation columns only; the whole rows come down when they are asked for
    cols = None if return_rows else [14, 19, 21, 31, 32]
    rows_list = []
    for c in chunks:
        got = (c.rows if cols is None else c.rows[:, :, cols].contiguous()).cpu().numpy()
        if cols is not None:
            full = np.zeros(got.shape[:2] + (kitti_eval.POSE_COLS,), np.float32)
            full[:, :, cols] = got
            got = full
        rows_list.extend(got[b] for b in range(got.shape[0]))
    rows_list = [r[:g.shape[0]] for r, g in zip(rows_list, labels_list)]
    result['summary'] = dict(error_summary(rows_list, labels_list), images=len(files), planes=int(planes_d.shape[0]), chunks=len(chunks))
    if return_rows:
        result['rows'] = rows_list
    return result


def ceiling_line(name, result):
    """ one table line of bin/polling_ceiling.py: the database, AP|R40 of the 3-D box, the BEV box and the image box at Easy / Moderate /
    Hard, and the error summary """
    s = result['summary']
    ap = lambda m: ' '.join('{:6.2f}'.format(result[(m, d)]['ap_r40']) for d in kitti_eval.DIFFICULTIES)  # noqa: E731
    return '{:<28s} {:6d} planes | 3d {} | bev {} | image {} | location median {:.3f} m max {:.3f} m | r_y max {:.4f} rad | NaN {:.2%}'.format(
        name, s['planes'], ap('3d'), ap('bev'), ap('image'), s['location_error_median_m'], s['location_error_max_m'], s['r_y_error_max_rad'], s['nan_share'])
