#!/usr/bin/env python3
"""
Measures the keypoint-label kernel and the ceiling of polling on one GPU, in ONE process: a synthetic dataset of the KITTI val split's
size -- `--images` (3 769) label files with the label statistics of tools/bench_kitti_eval.py's generator, every object rested on a row
of the shipped 100-plane database, its alpha and 2-D box made consistent with its pose -- under two calibrations: KITTI's own P2 and
the same P with a zero 4th column.

  (a) utils.label_prep.polling_ceiling per database (100 / 1k / 22k planes) and calibration: seconds, AP and the error summary
  (b) HIP events around each stage's launch alone, on the whole dataset as one chunk
  (c) the NumPy prepare_batch of that chunk against the gpp_label_prep_f64 launch (its results must be equal)

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_label_prep.jsonl and the tables of <out>/README.md between its two markers; <out> defaults to profiles/label_prep.
None of these figures is asserted anywhere: they are records.

    python tools/bench_label_prep.py [--out DIR] [--images 3769] [--rounds 3]
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_kitti_eval import launch_times, step_limit, write_dataset  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import gpp_utils, kitti_eval, synthetic  # noqa: E402
from keras_retinanet_3D.utils import label_prep as L  # noqa: E402

BEGIN, END = '<!-- bench_label_prep: begin -->', '<!-- bench_label_prep: end -->'
DATABASES = ('100', '1k', '22k')
NAMES = {0: 'Car', 1: 'Van', 2: 'DontCare', 3: 'Cyclist'}


def rest_on_planes(label_dir, calib_dirs, planes, seed=1):
    """ rewrites the label files of bench_kitti_eval's generator: every object that is no DontCare line is put on a row of `planes` (its
    y follows from x and z), alpha = r_y - atan2(x, z), the box is the prepared one under KITTI's P2 clipped to 375 x 1242; writes a
    calibration file per image into each of calib_dirs = {directory: P} """
    rng = np.random.default_rng(seed)
    planes = np.asarray(planes, np.float64)
    P2 = synthetic.KITTI_LIKE_P2
    n_cars = 0
    for f in sorted(os.listdir(label_dir)):
        path = os.path.join(label_dir, f)
        names, g = L.read_labels(path)
        for k in range(g.shape[0]):
            if g[k, 0] == 2:
                g[k, 1:4], g[k, 8:15] = (-1.0, -1.0, -10.0), (-1.0, -1.0, -1.0, -1000.0, -1000.0, -1000.0, -10.0)
                continue
            a, b, c, d = synthetic.canonical_plane(planes[rng.integers(0, planes.shape[0])])
            g[k, 11] = np.clip(g[k, 11], -0.45 * g[k, 13], 0.45 * g[k, 13])
            g[k, 12] = -(a * g[k, 11] + c * g[k, 13] + d) / b
            g[k, 3] = (g[k, 14] - math.atan2(g[k, 11], g[k, 13]) + math.pi) % (2 * math.pi) - math.pi
        g = np.array([[float('%.2f' % v) for v in row] for row in g]).reshape(-1, 16)
        mod = L.prepare(g, P2, strict=False)
        ok = mod[:, 19] >= 0
        g[ok, 4:8] = np.stack([np.clip(mod[ok, 4], 0, 1241), np.clip(mod[ok, 5], 0, 374), np.clip(mod[ok, 6], 0, 1241), np.clip(mod[ok, 7], 0, 374)], axis=1)
        n_cars += int((ok & (g[:, 0] == 0)).sum())
        with open(path, 'w') as out:
            for name, row in zip(names, g):
                out.write('{} {:.2f} {:d} '.format(name, row[1], int(row[2])) + ' '.join('%.2f' % v for v in row[3:15]) + '\n')
        for calib_dir, P in calib_dirs.items():
            with open(os.path.join(calib_dir, f), 'w') as out:
                out.write('P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P.ravel()) + '\n')
    return n_cars


def readme_tables(records):
    setup = records[0]
    lines = ['`tools/bench_label_prep.py`, one MI355X, one process; library `{}`.'.format(setup['library']), '',
             '{} images, {} labels ({} Cars in front of the camera), A = {}: {} chunk(s).  Objects rest on rows of the 100-plane database; '
             'labels carry two decimals, as KITTI\'s do.'.format(setup['images'], setup['labels'], setup['cars'], setup['A'], setup['chunks']), '',
             '| calibration | database | seconds (rounds) | 3-D AP R40 E / M / H | BEV AP R40 E / M / H | location median / max m | r_y max rad | NaN share |',
             '|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'polling_ceiling':
            lines.append('| {} | {} ({} planes) | {} | {} | {} | {:.3f} / {:.3f} | {:.4f} | {:.4f} |'.format(
                r['calibration'], r['database'], r['planes'], ' '.join('%.3f' % s for s in r['seconds']),
                ' / '.join('%.2f' % v for v in r['ap_3d']), ' / '.join('%.2f' % v for v in r['ap_bev']),
                r['summary']['location_error_median_m'], r['summary']['location_error_max_m'], r['summary']['r_y_error_max_rad'], r['summary']['nan_share']))
    lines += ['', '| launch alone (HIP events, the dataset as one chunk of B = {}, A = {}) | median us | min us |'.format(setup['images'], setup['A']), '|---|---|---|']
    for r in records:
        if r['what'] == 'launch_alone':
            lines.append('| `{}` | {} | {} |'.format(r['launch'], r['median_us'], r['min_us']))
    host = [r for r in records if r['what'] == 'numpy_prepare'][0]
    lines += ['', 'NumPy `prepare_batch` of the same chunk: {:.1f} ms (median of {}); its result and the kernel\'s are {}.'.format(
        host['median_ms'], host['runs'], 'equal' if host['equal'] else 'NOT EQUAL')]
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'label_prep'))
    ap.add_argument('--images', type=int, default=3769)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records = []

    def note(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    with tempfile.TemporaryDirectory() as root:
        label_dir = os.path.join(root, 'label_2')
        calibs = {'P2': synthetic.KITTI_LIKE_P2.copy(), 'P2, 4th column zero': synthetic.KITTI_LIKE_P2.copy()}
        calibs['P2, 4th column zero'][:, 3] = 0.0
        dirs = {name: os.path.join(root, 'calib_%d' % k) for k, name in enumerate(calibs)}
        for d in [label_dir] + list(dirs.values()):
            os.makedirs(d)
        with step_limit(420, 'the dataset'):
            _, n_labels, _ = write_dataset(label_dir, args.images)
            n_cars = rest_on_planes(label_dir, {dirs[name]: P for name, P in calibs.items()}, synthetic.load_plane_database('100'))
            files = sorted(os.listdir(label_dir))
            labels_list = [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in files]
            A = max(g.shape[0] for g in labels_list)
            step = kitti_eval.chunk_images(A, A)
            note({'what': 'setup', 'images': args.images, 'labels': n_labels, 'cars': n_cars, 'A': A, 'chunks': (args.images + step - 1) // step,
                  'library': hip.lib().gpp_version().decode()})
        for name in calibs:
            for db in DATABASES:
                planes = synthetic.load_plane_database(db)
                seconds, result = [], None
                for r in range(args.rounds + 1):                     # the first run is not timed
                    with step_limit(240, 'polling_ceiling {} {} round {}'.format(name, db, r)):
                        t0 = time.perf_counter()
                        result = L.polling_ceiling(label_dir, dirs[name], planes)
                        if r:
                            seconds.append(round(time.perf_counter() - t0, 4))
                note({'what': 'polling_ceiling', 'calibration': name, 'database': db, 'planes': int(planes.shape[0]), 'seconds': seconds,
                      'ap_3d': [round(result[('3d', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                      'ap_bev': [round(result[('bev', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                      'ap_image': [round(result[('image', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                      'aos': [round(result[('aos', d)]['aos_r40'], 4) for d in kitti_eval.DIFFICULTIES], 'summary': result['summary']})

        # the stages alone: the whole dataset as one chunk, KITTI's P2
        with step_limit(240, 'the launches alone'):
            B = len(files)
            P_list = [calibs['P2']] * B
            labels_d, counts_d, P_d, trig_d = L._upload(labels_list, P_list, A)
            shape = {'B': B, 'A': A}
            note(dict({'what': 'launch_alone', 'launch': 'gpp_label_prep_f64 (with the detection arrays)'}, **shape,
                      **launch_times(lambda: hip.label_prep(labels_d, counts_d, P_d, trig_d, L.CAR, True, True))))
            note(dict({'what': 'launch_alone', 'launch': 'gpp_label_prep_f64 (mod only)'}, **shape,
                      **launch_times(lambda: hip.label_prep(labels_d, counts_d, P_d, trig_d, 0, True, False))))
            mod_d, (boxes, dims, scores, det_labels, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, L.CAR, True, True)
            pinv_d = torch.as_tensor(np.tile(np.linalg.pinv(calibs['P2']).astype(np.float32), (B, 1, 1))).cuda()
            info_d = torch.as_tensor(np.tile(np.array([[1.0, 376.0, 1242.0]], np.float32), (B, 1))).cuda()
            keypoints = residuals = None
            for db in DATABASES:
                planes_d = torch.as_tensor(synthetic.load_plane_database(db).astype(np.float32)).cuda()
                note(dict({'what': 'launch_alone', 'launch': 'gpp_poll_f32, {} planes'.format(int(planes_d.shape[0]))}, **shape,
                          **launch_times(lambda: gpp_utils.fit_road_planes(boxes, dims, orient, pinv_d, planes_d), launches=30, skip=5)))
                keypoints, _, residuals = gpp_utils.fit_road_planes(boxes, dims, orient, pinv_d, planes_d)
            rows = torch.empty((B, A, hip.GPP_POSE_COLS), dtype=torch.float32, device='cuda')
            counts = torch.zeros((B,), dtype=torch.int32, device='cuda')
            pose = lambda: hip.check(hip.lib().gpp_pose_f32(hip.ptr(boxes), hip.ptr(dims), hip.ptr(scores), hip.ptr(det_labels), hip.ptr(orient),  # noqa: E731
                                                            hip.ptr(keypoints), hip.ptr(residuals), hip.ptr(info_d), B, A, 0.05, hip.ptr(rows),
                                                            hip.ptr(counts), hip.stream_ptr()), 'gpp_pose_f32')
            note(dict({'what': 'launch_alone', 'launch': 'gpp_pose_f32'}, **shape, **launch_times(pose)))
            note(dict({'what': 'launch_alone', 'launch': 'gpp_kitti_overlaps_f64 (D = A)'}, **shape,
                      **launch_times(lambda: hip.kitti_overlaps(rows, labels_d, counts_d))))
        with step_limit(240, 'the NumPy prepare'):
            packed, label_counts = kitti_eval.pack_labels(labels_list, A)
            P_all = np.stack(P_list)
            ms = []
            for _ in range(5):
                t0 = time.perf_counter()
                want = L.prepare_batch(packed, label_counts, P_all, det_types=L.CAR, own_box=True)
                ms.append((time.perf_counter() - t0) * 1e3)
            equal = np.array_equal(want[0], mod_d.cpu().numpy()) and all(
                np.array_equal(a, b.cpu().numpy()) for a, b in zip(want[1], (boxes, dims, scores, det_labels, orient)))
            note({'what': 'numpy_prepare', 'median_ms': round(statistics.median(ms), 2), 'runs': len(ms), 'equal': bool(equal), **shape})

    with open(os.path.join(args.out, 'bench_label_prep.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    readme = os.path.join(args.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# KITTI keypoint labels and the ceiling of polling: measurements\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN) + len(BEGIN)] + '\n' + readme_tables(records) + '\n' + text[text.index(END):]
        with open(readme, 'w') as f:
            f.write(text)
    if not [r for r in records if r['what'] == 'numpy_prepare'][0]['equal']:
        sys.exit('bench_label_prep: the kernel and the NumPy form differ')


if __name__ == '__main__':
    main()
