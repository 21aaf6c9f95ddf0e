#!/usr/bin/env python3
"""
Measures HOTA (csrc/hota_eval.hip, utils/hota_eval.py) on one GPU, in ONE process, on the two workloads of
tools/bench_mot_eval.py: `kitti`, the synthetic dataset of KITTI tracking's training size (21 sequences, about 8 000 frames), and `stress`,
32 frames of 128 labels x 128 rows.

  1. the three launches alone -- gpp_hota_potential, gpp_hota_match, gpp_hota_reduce -- on resident inputs (the overlaps and the codes of
     gpp_mot_assign computed once), HIP events around each launch, median of 50, with gpp_mot_assign beside them for scale; the bytes of
     the pair tables;
  2. the whole evaluate_sequences(device=True, hota=True) against the same call without HOTA (median of 7) and against the NumPy form on
     the same packed arrays (once), wall clock; whether the two forms are equal.

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_hota.jsonl (one JSON record per measurement) and <out>/tables.md; <out> defaults to profiles/hota.

    python tools/bench_hota.py [--out DIR] [--frames 8000] [--stress-frames 32]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_mot_eval import kitti_sized, median_us, step_limit, stress  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import hota_eval as H  # noqa: E402
from keras_retinanet_3D.utils import kitti_eval  # noqa: E402
from keras_retinanet_3D.utils import mot_eval as M  # noqa: E402
from keras_retinanet_3D.utils import pair_tables as PT  # noqa: E402


def launches(records, name, packed, params):
    dev = hip.require_device()
    N, A, D = packed.labels.shape[0], packed.labels.shape[1], packed.rows.shape[1]
    rows, ids = torch.as_tensor(packed.rows).to(dev), torch.as_tensor(packed.ids).to(dev)
    labels, counts = torch.as_tensor(packed.labels).to(dev), torch.as_tensor(packed.label_counts).to(dev)
    traj = torch.as_tensor(packed.traj).to(dev)
    prm = hip.MotParams(0, 0, params['min_overlap'], params['max_occlusion'], params['max_truncation'], params['min_height'])
    assert kitti_eval.chunk_images(D, A) >= N, 'one chunk'
    with step_limit(180, name + ': launches alone'):
        overlaps = hip.kitti_overlaps(rows, labels, counts)
        _, lout, rout, _ = hip.mot_assign(overlaps, labels, counts, rows, ids, prm)
        geo = PT.Geometry(packed, params, rows, ids, traj)
        run = H.DeviceRun(geo, N, dev)
        tab = geo.frame_tab.reshape(-1)

        def potential():
            run.workspace.zero_()                                               # (pass 1 adds: every repeat starts from zero)
            hip.hota_potential(overlaps, lout, rout, traj, geo.trk, 0, tab, geo.cells, geo.vecs, run.workspace)

        def match():                                                            # (hist grows with every repeat: the same atomics, other sums)
            return hip.hota_match(overlaps, lout, rout, traj, geo.trk, 0, tab, geo.cells, geo.vecs, run.workspace)

        potential()
        frame_hota = match()[1]
        zero_med, _ = median_us(lambda: run.workspace.zero_())
        for what, launch in (('gpp_mot_assign', lambda: hip.mot_assign(overlaps, labels, counts, rows, ids, prm)),
                             ('gpp_hota_potential', potential), ('gpp_hota_match', match),
                             ('gpp_hota_reduce', lambda: hip.hota_reduce(frame_hota, geo.seq_tab.reshape(-1), geo.cells, geo.vecs, run.workspace))):
            med, low = median_us(launch)
            if what == 'gpp_hota_potential':
                med, low = round(med - zero_med, 2), round(low - zero_med, 2)
            records.append({'what': 'launch', 'launch': what, 'workload': name, 'frames': N, 'D': D, 'A': A, 'sequences': len(packed.traj_ids),
                            'median_us': med, 'min_us': low, 'us_per_frame': round(med / max(N, 1), 3),
                            'note': 'includes the copy of its host table and the allocation of its outputs; potential: the median of '
                                    'zeroing the workspace ({} us) is subtracted'.format(zero_med)})
        records.append({'what': 'tables', 'workload': name, 'cells': geo.cells, 'counters': geo.vecs, 'workspace_bytes': int(run.workspace.numel()),
                        'largest_table': [int(v) for v in max(geo.seq_tab[:, 1:3].tolist(), key=lambda s: s[0] * s[1])]})


def whole(records, name, labels, tracks, params):
    with step_limit(900, name + ': evaluate_sequences'):
        M.evaluate_sequences(labels, tracks, device=True, hota=True)            # (warm: the library, the allocator)
        t_with, t_without = [], []
        for _ in range(7):                                                      # (every leg ends in a download: the clock sees finished work)
            t0 = time.perf_counter()
            dev = M.evaluate_sequences(labels, tracks, device=True, hota=True)
            t_with.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            M.evaluate_sequences(labels, tracks, device=True)
            t_without.append(time.perf_counter() - t0)
        packed = M.pack_sequences(labels, tracks)
        t0 = time.perf_counter()
        plain = M.evaluate_packed_np(packed, params)
        t_plain = time.perf_counter() - t0
        t0 = time.perf_counter()
        host = H.add_hota_np(plain, packed, params)
        t_hota = time.perf_counter() - t0
    same = dev['all'] == host['all'] and dev['sequences'] == host['sequences'] and \
        all(np.array_equal(dev['hota_frames'][k], host['hota_frames'][k]) for k in dev['hota_frames']) and \
        all(np.array_equal(a[k], b[k]) for a, b in zip(dev['hota_pairs'], host['hota_pairs']) for k in a)
    records.append({'what': 'whole', 'workload': name, 'frames': int(packed.labels.shape[0]),
                    'device_with_hota_ms': round(statistics.median(t_with) * 1e3, 1), 'device_without_hota_ms': round(statistics.median(t_without) * 1e3, 1),
                    'numpy_clear_mot_ms': round(t_plain * 1e3, 1), 'numpy_hota_on_top_ms': round(t_hota * 1e3, 1), 'equal': bool(same),
                    'hota': {k: host['all']['hota'][k] for k in H.RATIOS}})


def tables(records):
    out = ['| launch | workload | frames | D | A | median us | min us | us per frame |', '|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'launch':
            out.append('| {launch} | {workload} | {frames} | {D} | {A} | {median_us} | {min_us} | {us_per_frame} |'.format(**r))
    out += ['', '| pair tables | cells | counters | workspace bytes | largest table |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'tables':
            out.append('| {workload} | {cells} | {counters} | {workspace_bytes} | {largest_table} |'.format(**r))
    out += ['', '| evaluate_sequences | frames | device with HOTA ms | device without ms | NumPy CLEAR-MOT ms | NumPy HOTA on top ms | equal |',
            '|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'whole':
            out.append('| {workload} | {frames} | {device_with_hota_ms} | {device_without_hota_ms} | {numpy_clear_mot_ms} | {numpy_hota_on_top_ms} | {equal} |'.format(**r))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hota'))
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
    with open(os.path.join(args.out, 'bench_hota.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    with open(os.path.join(args.out, 'tables.md'), 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
