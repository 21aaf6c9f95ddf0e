#!/usr/bin/env python
"""
Measures the offline smoother (csrc/track_smooth.hip, utils/track_smooth.py) on one GPU, in ONE process.

  set 1   KITTI tracking's training size -- 21 synthetic sequences, 7 991 frames, the generator of tools/bench_mot_eval.py, its tracker ids
          as the finished run --: the two launches' time (torch.profiler), the whole device call against the NumPy form in this
          process, the workspace's bytes.  Every call timed returned the NumPy form's words.
  set 2   tools/bench_track_kf.py's synthetic_set, seeds 0 - 2, 'maha' 3.0 with its ego records: position RMS against the scene's truth
          raw, filtered (the tracker's 'smooth') and smoothed, and FN FRAG MOTA HOTA DetRe LocA with and without the smoother through
          sections 4.29 - 4.30 against the truth of EVERY frame a car is in range, the missed ones included.  No GPU is needed for this
          set (--host).

The filter is given the noise model that made the data; no real checkpoint or KITTI sequence has been seen.  Nothing is asserted.

    python tools/bench_track_smooth.py [--out profiles/track_smooth] [--host] [--repeats 5]
"""
import argparse
import json
import math
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from keras_retinanet_3D.utils import mot_eval  # noqa: E402
from keras_retinanet_3D.utils import track as T  # noqa: E402
from keras_retinanet_3D.utils import track_smooth as S  # noqa: E402

MAX_GAP = 2


def kitti_sized_run():
    """ the 21 sequences of tools/bench_mot_eval.kitti_sized(7991) as one finished run: rows (N, D, 36), ids (N, D), seq_start """
    import bench_mot_eval as BM
    _, tracks = BM.kitti_sized(7991)
    frames = [(r, i) for rows, ids in tracks for r, i in zip(rows, ids)]
    D = max(len(r) for r, _ in frames)
    rows = np.full((len(frames), D, 36), -1.0, np.float32)
    ids = np.full((len(frames), D), -1, np.int32)
    for f, (r, i) in enumerate(frames):
        rows[f, :len(r)], ids[f, :len(r)] = r, i
    seq_start = np.concatenate([[0], np.cumsum([len(t[0]) for t in tracks])])
    return rows, ids, seq_start


def set_1(records, noise, repeats):
    import torch
    from keras_retinanet_3D.backend import hip
    rows, ids, seq_start = kitti_sized_run()
    t0 = time.perf_counter()
    index = S.segments_of(ids, seq_start, MAX_GAP, rows)
    t_index = time.perf_counter() - t0
    length = np.diff(index.seg_start)
    t0 = time.perf_counter()
    want = S.smooth_np(rows, index, noise)
    t_np = time.perf_counter() - t0
    dev = torch.as_tensor(rows).cuda()
    calls = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = S.smooth_device(dev, index, noise)
        torch.cuda.synchronize()
        calls.append(time.perf_counter() - t0)
    same = all(np.array_equal(g.cpu().numpy()[..., [c for c in range(g.shape[-1]) if g.shape[-1] != 36 or c != 25]],
                              w[..., [c for c in range(w.shape[-1]) if w.shape[-1] != 36 or c != 25]], equal_nan=True) for g, w in zip(got, want))
    kernels = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(repeats):
                S.smooth_device(dev, index, noise)
            torch.cuda.synchronize()
        for e in prof.key_averages():
            name = re.search(r'track_smooth_\w+(<\w+>)?', e.key)
            if name:
                us = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
                kernels[name.group(0)] = round(us / max(e.count, 1), 1)
    except Exception as e:                                               # the profiler is a convenience: without it the number is not reported
        kernels = {'not measured': repr(e)[:80]}
    records.append({'what': 'set 1', 'frames': int(rows.shape[0]), 'D': int(rows.shape[1]), 'sequences': len(seq_start) - 1,
                    'segments': int(length.size), 'segments_of_2_or_more': int((length >= 2).sum()), 'cells': int(index.cell_row.size),
                    'fills': int((index.cell_row < 0).sum()), 'longest_segment': int(length.max()), 'max_gap': MAX_GAP,
                    'segments_of_ms': round(1e3 * t_index, 2), 'numpy_form_ms': round(1e3 * t_np, 2),
                    'device_call_ms_first': round(1e3 * calls[0], 2), 'device_call_ms_median': round(1e3 * float(np.median(calls[1:])), 3),
                    'kernel_us': kernels, 'workspace_bytes': hip.track_smooth_workspace_bytes(rows.shape[0], length.size, index.cell_row.size),
                    'equals_numpy_form': bool(same)})


def truth_of(seed):
    """ synthetic_set's scene without noise and without misses -- the same random stream: every draw is made, with a scale of 0 and
    against a probability of 0 -- -> per frame {car: (x, z)}, and the labels of every car in range """
    import bench_track_kf as BK
    import bench_track_optimal as BO
    noise, BK.NOISE = BK.NOISE, dict(BK.NOISE, radial=(0.0, 0.0), tangential=(0.0, 0.0))
    try:
        frames, _, gts = BK.synthetic_set(seed, miss=0.0)
    finally:
        BK.NOISE = noise
    where = [{int(k): (float(r[19]), float(r[21])) for r, k in zip(rows, g) if k >= 0} for rows, g in zip(frames, gts)]
    return where, BO.labels_of(frames, gts)


def rms(rows, gts, where, ids):
    err = [(float(r[19]) - where[f][int(k)][0]) ** 2 + (float(r[21]) - where[f][int(k)][1]) ** 2
           for f in range(len(rows)) for r, k, i in zip(rows[f], gts[f], ids[f]) if k >= 0 and i >= 0]
    return round(math.sqrt(sum(err) / max(len(err), 1)), 4), len(err)


def set_2(records, host):
    import bench_track_kf as BK
    option = {'metric': 'maha', 'threshold': 3.0, 'filter': 'kalman', 'noise': BK.NOISE}
    for seed in (0, 1, 2):
        frames, ego, gts = BK.synthetic_set(seed)
        where, labels = truth_of(seed)
        assert all(set(int(k) for k in g if k >= 0) <= set(w) for g, w in zip(gts, where))
        raw, ids, hits = T.track_rows_np(frames, option, ego=ego)[:3]
        filtered = T.track_rows_np(frames, dict(option, smooth=True), ego=ego)[0]
        merged = S.smooth_tracks(frames, ids, hits, BK.NOISE, MAX_GAP, ego=ego, host=host)
        smoothed = [r[:frames.shape[1]] for r in merged[0]]
        rec = {'what': 'set 2', 'seed': seed, 'frames': len(frames), 'rows': int(sum((g >= 0).sum() for g in gts)), 'fills': merged[3],
               'labels': int(sum(len(x) for x in labels[0])), 'rms_raw_m': rms(raw, gts, where, ids)[0],
               'rms_filtered_m': rms(filtered, gts, where, ids)[0], 'rms_smoothed_m': rms(smoothed, gts, where, ids)[0]}
        for name, (rows_, ids_) in (('tracker', (list(raw), list(ids))), ('filtered', (list(filtered), list(ids))), ('rts', (merged[0], merged[1]))):
            score = mot_eval.evaluate_sequences([labels], [(rows_, ids_)], metric='bev', hota=True)['all']
            rec[name] = {'FN': int(score['fn']), 'FP': int(score['fp']), 'FRAG': int(score['frag']), 'IDS': int(score['ids']),
                         'MOTA': round(score['mota'], 4), 'MOTP': round(score['motp'], 4), 'HOTA': round(float(score['hota']['hota']), 4),
                         'DetRe': round(float(score['hota']['detre']), 4), 'LocA': round(float(score['hota']['loca']), 4)}
        records.append(rec)


def tables(records):
    out = []
    for r in records:
        if r['what'] == 'set 1':
            out += ['| set 1 | value |', '|---|---|'] + ['| {} | {} |'.format(k, v) for k, v in r.items() if k != 'what'] + ['']
    out += ['| seed | rows | fills | RMS raw m | RMS filtered m | RMS smoothed m | run | FN | FP | FRAG | IDS | MOTA | MOTP | HOTA | DetRe | LocA |',
            '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'set 2':
            for name in ('tracker', 'filtered', 'rts'):
                out.append('| {seed} | {rows} | {fills} | {rms_raw_m} | {rms_filtered_m} | {rms_smoothed_m} | '.format(**r) + name +
                           ' | {FN} | {FP} | {FRAG} | {IDS} | {MOTA} | {MOTP} | {HOTA} | {DetRe} | {LocA} |'.format(**r[name]))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_smooth'))
    ap.add_argument('--host', action='store_true', help='set 2 only, on the NumPy form: no GPU')
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    import bench_track_kf as BK
    records = []
    if not args.host:
        set_1(records, BK.NOISE, args.repeats)
        print(json.dumps(records[-1]), flush=True)
    set_2(records, args.host)
    os.makedirs(args.out, exist_ok=True)
    name = 'bench_track_smooth_host' if args.host else 'bench_track_smooth'
    with open(os.path.join(args.out, name + '.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    with open(os.path.join(args.out, 'tables_host.md' if args.host else 'tables.md'), 'w') as f:
        f.write(tables(records))
    print(tables(records))


if __name__ == '__main__':
    main()
