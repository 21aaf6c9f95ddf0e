#!/usr/bin/env python3
"""
Measures the tracking score (csrc/mot_eval.hip, utils/mot_eval.py) on one GPU, in ONE process, on two workloads:

  kitti    a synthetic dataset of KITTI tracking's training size: 21 sequences, about 8 000 frames, 5 - 15 cars per frame that drift over
           the image, rows that follow them with jitter, misses, clutter and ids that change hands;
  stress   32 frames of 128 labels x 128 rows in which every row overlaps two labels alike (tests/mot_oracle.py's dense frame).

  1. the launches alone -- gpp_kitti_overlaps_f64 (for scale), gpp_mot_assign, gpp_mot_clear -- on resident inputs, HIP events around each
     launch, median of 50;
  2. the whole evaluate_sequences(device=True) (packing, upload, three launches per chunk, download; median of 7) against the NumPy
     form (once), wall clock;
  3. the assignment alone on the same cost matrices: assign_np against a per-frame scipy.optimize.linear_sum_assignment loop, and whether
     the totals agree.

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_mot_eval.jsonl (one JSON record per measurement) and <out>/tables.md; <out> defaults to profiles/mot.

    python tools/bench_mot_eval.py [--out DIR] [--frames 8000] [--stress-frames 32]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import kitti_eval  # noqa: E402
from keras_retinanet_3D.utils import mot_eval as M  # noqa: E402


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_mot_eval: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def boxes_to_labels(x1, y1, w, h, kind=0.0):
    n = x1.shape[0]
    out = np.zeros((n, 16))
    out[:, 0], out[:, 4], out[:, 5], out[:, 6], out[:, 7] = kind, x1, y1, x1 + w, y1 + h
    out[:, 8], out[:, 9], out[:, 10], out[:, 11], out[:, 12], out[:, 13] = 1.5, w / 32.0, h / 16.0, x1 / 16.0, 1.65, 20.0 + y1 / 8.0
    return out


def rows_of(labels):
    line = labels.copy()
    line[:, 0], line[:, 15] = 0.0, 1.0
    return kitti_eval.rows_from_results(line)


def sequence(seed, frames):
    """ one sequence: 5 - 15 cars, a tenth of the rows missing, two clutter rows, ids that change hands now and then """
    rng = np.random.default_rng(seed)
    cars = int(rng.integers(5, 16))
    x, y = rng.uniform(0.0, 1100.0, cars), rng.uniform(150.0, 250.0, cars)
    w, h = rng.uniform(60.0, 200.0, cars), rng.uniform(30.0, 110.0, cars)
    vx = rng.uniform(-2.0, 2.0, cars)
    tracker = np.arange(cars) + 1
    labs, tids, rows, ids = [], [], [], []
    for f in range(frames):
        if rng.random() < 0.02:
            a, b = rng.choice(cars, 2, replace=False)
            tracker[a], tracker[b] = tracker[b], tracker[a]
        here = x + vx * f
        labs.append(boxes_to_labels(here, y, w, h))
        tids.append(np.arange(cars))
        keep = np.flatnonzero(rng.random(cars) >= 0.1)
        seen = boxes_to_labels(here[keep] + rng.normal(0.0, 4.0, keep.size), y[keep] + rng.normal(0.0, 3.0, keep.size), w[keep], h[keep])
        clutter = boxes_to_labels(rng.uniform(0.0, 1100.0, 2), rng.uniform(150.0, 250.0, 2), np.full(2, 80.0), np.full(2, 50.0))
        rows.append(rows_of(np.concatenate([seen, clutter])))
        ids.append(np.concatenate([tracker[keep], [900, 901]]).astype(np.int32))
    return (labs, tids), (rows, ids)


def kitti_sized(total_frames):
    rng = np.random.default_rng(2)
    share = rng.uniform(0.4, 2.6, 21)
    lengths = np.maximum(1, (share / share.sum() * total_frames).astype(int))
    scenes = [sequence(100 + s, int(n)) for s, n in enumerate(lengths)]
    return [s[0] for s in scenes], [s[1] for s in scenes]


def stress(frames):
    """ per frame 128 labels 16 px apart, 64 px wide, and 128 rows 8 px further: a row overlaps two labels by 56 / 72 each """
    labs, tids, rows, ids = [], [], [], []
    for f in range(frames):
        rng = np.random.default_rng(500 + f)
        k = np.arange(128)
        labs.append(boxes_to_labels(16.0 * k, np.full(128, 100.0), np.full(128, 64.0), np.full(128, 64.0)))
        tids.append(k)
        at = rng.permutation(128) * 16.0 + rng.integers(0, 3, 128) * 8.0
        rows.append(rows_of(boxes_to_labels(at, np.full(128, 100.0), np.full(128, 64.0), np.full(128, 64.0))))
        ids.append((k + 1).astype(np.int32))
    return [(labs, tids)], [(rows, ids)]


def median_us(launch, n=50, warm=5):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0)
    return round(statistics.median(us), 2), round(min(us), 2)


def launches(records, name, packed, params):
    dev = hip.require_device()
    N, A, D = packed.labels.shape[0], packed.labels.shape[1], packed.rows.shape[1]
    rows, ids = torch.as_tensor(packed.rows).to(dev), torch.as_tensor(packed.ids).to(dev)
    labels, counts = torch.as_tensor(packed.labels).to(dev), torch.as_tensor(packed.label_counts).to(dev)
    traj = torch.as_tensor(packed.traj).to(dev)
    prm = hip.MotParams(0, 0, params['min_overlap'], params['max_occlusion'], params['max_truncation'], params['min_height'])
    step = kitti_eval.chunk_images(D, A)
    assert step >= N, 'one chunk'
    n_traj = max(t.size for t in packed.traj_ids)
    with step_limit(120, name + ': launches alone'):
        overlaps = hip.kitti_overlaps(rows, labels, counts)
        res = hip.mot_assign(overlaps, labels, counts, rows, ids, prm)
        for what, launch in (('gpp_kitti_overlaps_f64', lambda: hip.kitti_overlaps(rows, labels, counts)),
                             ('gpp_mot_assign', lambda: hip.mot_assign(overlaps, labels, counts, rows, ids, prm)),
                             ('gpp_mot_clear', lambda: hip.mot_clear(res[0], res[1], traj, ids, res[3], packed.seq_start, n_traj))):
            med, low = median_us(launch)
            records.append({'what': 'launch', 'launch': what, 'workload': name, 'frames': N, 'D': D, 'A': A, 'sequences': len(packed.traj_ids),
                            'median_us': med, 'min_us': low, 'us_per_frame': round(med / max(N, 1), 3),
                            'note': 'includes the allocation of its outputs'})


def whole(records, name, labels, tracks, params):
    with step_limit(300, name + ': evaluate_sequences'):
        M.evaluate_sequences(labels, tracks, device=True)                       # (warm: the library, the allocator)
        t_dev, t_pack, t_dev_packed = [], [], []
        for _ in range(7):                                                      # (every leg ends in a download: the clock sees finished work)
            t0 = time.perf_counter()
            dev = M.evaluate_sequences(labels, tracks, device=True)
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            packed = M.pack_sequences(labels, tracks)
            t_pack.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            M.evaluate_packed_device(packed, params)
            t_dev_packed.append(time.perf_counter() - t0)
        t_dev, t_pack, t_dev_packed = (statistics.median(t) for t in (t_dev, t_pack, t_dev_packed))
        t0 = time.perf_counter()
        host = M.evaluate_packed_np(packed, params)
        t_host = time.perf_counter() - t0
    same = dev['all'] == host['all'] and dev['sequences'] == host['sequences'] and \
        all(np.array_equal(dev['frames'][k], host['frames'][k]) for k in dev['frames'])
    records.append({'what': 'whole', 'workload': name, 'frames': int(packed.labels.shape[0]), 'device_ms': round(t_dev * 1e3, 1),
                    'packing_ms': round(t_pack * 1e3, 1), 'device_after_packing_ms': round(t_dev_packed * 1e3, 1),
                    'numpy_after_packing_ms': round(t_host * 1e3, 1), 'equal': bool(same), 'all': host['all']})
    # ---- the assignment alone, on the same matrices
    from scipy.optimize import linear_sum_assignment
    matrices = []
    for f in range(packed.labels.shape[0]):
        c = int(packed.label_counts[f])
        o = kitti_eval.image_overlaps(packed.rows[f], packed.labels[f, :c])[0]
        status = M.label_status(packed.labels[f, :c])
        live = (packed.rows[f][:, 14] >= 0) & (packed.ids[f] >= 0)
        matrices.append(M.cost_matrix_np(o, status, live)[0])
    t0 = time.perf_counter()
    ours = [M.assign_np(c)[1] for c in matrices]
    t_np = time.perf_counter() - t0
    t0 = time.perf_counter()
    theirs = []
    for c in matrices:
        r, k = linear_sum_assignment(c)
        theirs.append(int(c[r, k].sum()))
    t_scipy = time.perf_counter() - t0
    records.append({'what': 'assignment', 'workload': name, 'frames': len(matrices), 'assign_np_ms': round(t_np * 1e3, 1),
                    'scipy_loop_ms': round(t_scipy * 1e3, 1), 'totals_equal': ours == theirs,
                    'device_totals_equal': dev['frames']['counts'][:, 5].tolist() == theirs})


def tables(records):
    out = ['| launch | workload | frames | D | A | median us | min us | us per frame |', '|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'launch':
            out.append('| {launch} | {workload} | {frames} | {D} | {A} | {median_us} | {min_us} | {us_per_frame} |'.format(**r))
    out += ['', '| evaluate_sequences | frames | device, whole ms | packing ms | device after packing ms | NumPy after packing ms | equal |',
            '|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'whole':
            out.append('| {workload} | {frames} | {device_ms} | {packing_ms} | {device_after_packing_ms} | {numpy_after_packing_ms} | {equal} |'.format(**r))
    out += ['', '| assignment alone | frames | assign_np ms | scipy loop ms | totals equal | device totals equal |', '|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'assignment':
            out.append('| {workload} | {frames} | {assign_np_ms} | {scipy_loop_ms} | {totals_equal} | {device_totals_equal} |'.format(**r))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mot'))
    ap.add_argument('--frames', type=int, default=8000)
    ap.add_argument('--stress-frames', type=int, default=32)
    args = ap.parse_args()
    hip.require_device()
    os.makedirs(args.out, exist_ok=True)
    params = M.check_params()
    records = []
    for name, (labels, tracks) in (('kitti', kitti_sized(args.frames)), ('stress', stress(args.stress_frames))):
        launches(records, name, M.pack_sequences(labels, tracks), params)
        whole(records, name, labels, tracks, params)
    with open(os.path.join(args.out, 'bench_mot_eval.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    with open(os.path.join(args.out, 'tables.md'), 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
