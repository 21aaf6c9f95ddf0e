#!/usr/bin/env python3
"""
Measures utils.kitti_eval.evaluate_kitti on one GPU, in ONE process: a synthetic dataset of the KITTI val split's size -- `--images`
(3 769) label files of about 8 labels each and up to 100 detection rows per image, jittered around the labels --

  (a) evaluate_kitti(label_dir, rows=rows, device=True)     overlaps and matching in csrc/kitti_eval.hip
  (b) evaluate_kitti(label_dir, rows=rows)                  NumPy

Both parse the same label files.  (a) and (b) alternate `--rounds` times in the same process on the same box (boxes differ by several
percent: numbers of two runs cannot be compared); their integer results, thresholds and APs must be equal, AOS within 1e-9.  Also: HIP
events around each of the launches alone, on one chunk.  Every GPU step runs under a time limit of its own (SIGALRM: the process ends
there, nothing more is started).  Writes <out>/bench_kitti_eval.jsonl and the tables of <out>/README.md between its two markers (the
bench.py A/B of the same README is written by hand from tools/ab_bench.sh's output); <out> defaults to profiles/kitti_eval.

    python tools/bench_kitti_eval.py [--out DIR] [--images 3769] [--rounds 3]
"""
import argparse
import json
import math
import os
import signal
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import kitti_eval  # noqa: E402

BEGIN, END = '<!-- bench_kitti_eval: begin -->', '<!-- bench_kitti_eval: end -->'


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_kitti_eval: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def write_dataset(label_dir, n_images, seed=0):
    """ label files and, per image, (100, 36) float32 rows: three detections in four lie close to a label, the rest anywhere near one """
    rng = np.random.default_rng(seed)
    names = ('Car', 'Car', 'Car', 'Car', 'Van', 'DontCare', 'Cyclist')
    rows_list, n_labels, n_dets = [], 0, 0
    for i in range(n_images):
        A = int(np.clip(rng.poisson(8), 1, 24))
        D = int(rng.integers(20, 101))
        lab = np.zeros((A, 15))
        lab[:, 0], lab[:, 1], lab[:, 2] = rng.choice([0.0, 0.1, 0.2, 0.4], A), rng.integers(0, 4, A), rng.uniform(-math.pi, math.pi, A)
        lab[:, 3], lab[:, 4] = rng.uniform(0, 1100, A), rng.uniform(120, 250, A)
        lab[:, 5], lab[:, 6] = lab[:, 3] + rng.uniform(30, 140, A), lab[:, 4] + rng.uniform(20, 110, A)
        lab[:, 7], lab[:, 8], lab[:, 9] = rng.uniform(1.4, 1.8, A), rng.uniform(1.5, 2.0, A), rng.uniform(3.0, 5.0, A)
        lab[:, 10], lab[:, 11], lab[:, 12] = rng.uniform(-25, 25, A), rng.uniform(1.2, 2.0, A), rng.uniform(5, 70, A)
        lab[:, 13] = rng.uniform(-math.pi, math.pi, A)
        kinds = rng.integers(0, len(names), A)
        with open(os.path.join(label_dir, '%06d.txt' % i), 'w') as f:
            for k in range(A):
                f.write('{} {:.2f} {:d} '.format(names[kinds[k]], lab[k, 0], int(lab[k, 1])) + ' '.join('%.2f' % v for v in lab[k, 2:14]) + '\n')
        g = lab[rng.integers(0, A, D)]
        j = np.where(rng.random(D) < 0.75, 0.12, 3.0)[:, None]
        rows = np.full((100, 36), -1.0, np.float32)
        rows[:D] = 0.0
        rows[:D, 12] = np.sort(rng.uniform(0.05, 1.0, D))[::-1]
        rows[:D, 25] = g[:, 2] + rng.uniform(-0.3, 0.3, D)
        rows[:D, 26:30] = g[:, 3:7] + rng.uniform(-1, 1, (D, 4)) * j * 12
        rows[:D, 30], rows[:D, 17], rows[:D, 18] = (g[:, 7:10] * rng.uniform(0.96, 1.04, (D, 3))).T
        rows[:D, 19], rows[:D, 31], rows[:D, 21] = (g[:, 10:13] + rng.uniform(-1, 1, (D, 3)) * j * (1.0, 0.3, 1.0)).T
        rows[:D, 32] = g[:, 13] + rng.uniform(-0.4, 0.4, D) * j[:, 0]
        rows_list.append(rows)
        n_labels, n_dets = n_labels + A, n_dets + D
    return rows_list, n_labels, n_dets


def same(got, want):
    for key, entry in want.items():
        for name, value in entry.items():
            if name.startswith('aos'):
                if not abs(got[key][name] - value) <= 1e-9:
                    return False
            elif not np.array_equal(got[key][name], value):
                return False
    return True


def launch_times(fn, launches=120, skip=20):
    us = []
    for it in range(launches):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        e[1].synchronize()
        if it >= skip:
            us.append(e[0].elapsed_time(e[1]) * 1e3)          # (includes the allocation of the result tensors)
    return {'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'launches': len(us)}


def readme_tables(records):
    setup = records[0]
    legs = {(r['path'], r['round']): r for r in records if r['what'] == 'evaluate_kitti'}
    rounds = sorted({r for _, r in legs})
    lines = ['`tools/bench_kitti_eval.py`, one MI355X, one process; library `{}`.'.format(setup['library']), '',
             '{} images, {} labels, {} detection rows (D = {}, A = {}: {} chunk(s) of up to {} images); the two results are {}; '
             'AP|R40 of the 3-D box at Moderate: {:.2f}.'.format(setup['images'], setup['labels'], setup['detections'], setup['D'], setup['A'], setup['chunks'],
                                                                  setup['chunk_images'], 'equal' if setup['device_equals_host'] else 'NOT EQUAL', setup['ap_3d_moderate']), '',
             '| round | `evaluate_kitti(device=True)` s | `evaluate_kitti(device=False)` s |', '|---|---|---|']
    for r in rounds:
        lines.append('| {} | {:.3f} | {:.3f} |'.format(r, legs[('device', r)]['seconds'], legs[('host', r)]['seconds']))
    lines += ['', 'Reading the {} label files alone (both legs pay it): {:.3f} s.'.format(setup['images'], [r for r in records if r['what'] == 'labels_alone'][0]['seconds']), '',
              '| launch alone (HIP events, one chunk of B = {}) | median us | min us |'.format([r for r in records if r['what'] == 'launch_alone'][0]['B']), '|---|---|---|']
    for r in records:
        if r['what'] == 'launch_alone':
            lines.append('| `{}` | {} | {} |'.format(r['launch'], r['median_us'], r['min_us']))
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kitti_eval'))
    ap.add_argument('--images', type=int, default=3769)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records = []

    def note(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    with tempfile.TemporaryDirectory() as label_dir:
        with step_limit(420, 'the dataset and one untimed run of each leg'):
            rows_list, n_labels, n_dets = write_dataset(label_dir, args.images)
            want = kitti_eval.evaluate_kitti(label_dir, rows=rows_list)
            got = kitti_eval.evaluate_kitti(label_dir, rows=rows_list, device=True)
            labels_list = [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in sorted(os.listdir(label_dir))]
            A = max(g.shape[0] for g in labels_list)
            step = kitti_eval.chunk_images(100, A)
            note({'what': 'setup', 'images': args.images, 'labels': n_labels, 'detections': n_dets, 'D': 100, 'A': A, 'chunk_images': step,
                  'chunks': (args.images + step - 1) // step, 'device_equals_host': bool(same(got, want)),
                  'ap_3d_moderate': round(want[('3d', 'moderate')]['ap_r40'], 4), 'ap_image_moderate': round(want[('image', 'moderate')]['ap_r40'], 4),
                  'library': hip.lib().gpp_version().decode()})

        for r in range(args.rounds):
            for name, device in (('device', True), ('host', False)):
                with step_limit(300, '{} round {}'.format(name, r + 1)):
                    t0 = time.perf_counter()
                    kitti_eval.evaluate_kitti(label_dir, rows=rows_list, device=device)
                    dt = time.perf_counter() - t0
                note({'what': 'evaluate_kitti', 'path': name, 'round': r + 1, 'seconds': round(dt, 4), 'images_per_s': round(args.images / dt, 1)})

        with step_limit(120, 'reading the labels alone'):
            t0 = time.perf_counter()
            for f in sorted(os.listdir(label_dir)):
                kitti_eval.read_label_file(os.path.join(label_dir, f))
            note({'what': 'labels_alone', 'seconds': round(time.perf_counter() - t0, 4)})

    with step_limit(120, 'the launches alone'):
        B = min(step, args.images)
        chunk = kitti_eval.upload_chunk(np.stack(rows_list[:B]), labels_list[:B])
        mo = (0.7, 0.7, 0.7)
        shape = {'B': B, 'D': 100, 'A': int(chunk.labels.shape[1])}
        note(dict({'what': 'launch_alone', 'launch': 'gpp_kitti_overlaps_f64'}, **shape,
                  **launch_times(lambda: hip.kitti_overlaps(chunk.rows, chunk.labels, chunk.label_counts))))
        note(dict({'what': 'launch_alone', 'launch': 'gpp_kitti_stats_f64, pass 1'}, **shape,
                  **launch_times(lambda: hip.kitti_stats(chunk.rows, chunk.labels, chunk.label_counts, chunk.overlaps, mo))))
        thr = np.tile(np.linspace(0.95, 0.05, 41, dtype=np.float32), (3, 3, 1))
        thr_d, n_d = torch.as_tensor(thr).cuda(), torch.full((3, 3), 41, dtype=torch.int32, device='cuda')
        note(dict({'what': 'launch_alone', 'launch': 'gpp_kitti_stats_f64, pass 2 (T = 41)'}, **shape,
                  **launch_times(lambda: hip.kitti_stats(chunk.rows, chunk.labels, chunk.label_counts, chunk.overlaps, mo, thr_d, n_d))))

    with open(os.path.join(args.out, 'bench_kitti_eval.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    readme = os.path.join(args.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# KITTI object benchmark on the device: measurements\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN) + len(BEGIN)] + '\n' + readme_tables(records) + '\n' + text[text.index(END):]
        with open(readme, 'w') as f:
            f.write(text)
    if not records[0]['device_equals_host']:
        sys.exit('bench_kitti_eval: evaluate_kitti(device=True) != evaluate_kitti(device=False)')


if __name__ == '__main__':
    main()
