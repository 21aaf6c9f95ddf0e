#!/usr/bin/env python3
"""
Measures the tracker (csrc/track.hip, RetinaNet3D(pose=True, track=...)) on one GPU, in ONE process:

  1. the launch alone: one sequence of N = 8 frames (and of N = 1) of D = 100 rows -- 100 cars on a 10 x 10 grid 12 m apart, a few
     centimetres of jitter per frame --, entered with 0, 50 and 128 occupied slots, per metric; HIP events around each launch, median of
     200.  The launch always goes from the same entry state to a second buffer, so every repetition does the same work;
  2. at B = 8, resnet50, the 1k plane database, 402 x 1333: ms per predict_tracks_on_frames call against predict_poses_on_frames of the
     same model, alternating in the same process on the same box (boxes differ by several percent: numbers of two runs cannot be compared);
  3. track_rows_np (the NumPy form) on the rows of such a call.

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_track.jsonl (one JSON record per measurement) and <out>/launch_tables.md (the tables that <out>/README.md quotes); <out>
defaults to profiles/track.

    python tools/bench_track.py [--out DIR] [--steps 30] [--warmup 5] [--rounds 3] [--dtype f16x3]
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

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.models import weights as W  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402
from keras_retinanet_3D.utils import track as T  # noqa: E402

THRESHOLDS = {'bev': 0.1, '3d': 0.1, 'dist': 2.0}


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_track: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def grid(n_rows, n_live, seed, jitter=0.03):
    """ (n_rows, 36) float32: car k on a grid 12 m apart (16 per line), the first n_live rows live; only the columns the tracker reads """
    rng = np.random.default_rng(seed)
    rows = np.full((n_rows, 36), -1.0, np.float32)
    k = np.arange(n_live)
    live = np.zeros((n_live, 36), np.float32)
    live[:, 12] = np.linspace(0.99, 0.06, n_live)
    live[:, 17], live[:, 18], live[:, 30], live[:, 31] = 1.6, 4.0, 1.5, 1.65
    live[:, 19] = -90.0 + 12.0 * (k % 16) + rng.normal(0.0, jitter, n_live)
    live[:, 21] = 8.0 + 12.0 * (k // 16) + rng.normal(0.0, jitter, n_live)
    live[:, 32] = 0.3 * np.sin(k) + rng.normal(0.0, 0.01, n_live)
    rows[:n_live] = live
    return rows


def median_us(launch, n=200, warm=20):
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
    return statistics.median(us), min(us)


def launches_alone(records):
    dev = hip.require_device()
    work = torch.empty((hip.track_workspace_bytes(1),), dtype=torch.uint8, device=dev)
    for N in (8, 1):
        host = np.stack([grid(100, 100, 10 + f) for f in range(N)])
        rows = torch.as_tensor(host).to(dev)
        out, ids, hits = torch.empty_like(rows), torch.empty((N, 100), dtype=torch.int32, device=dev), torch.empty((N, 100), dtype=torch.int32, device=dev)
        for metric in T.METRICS:
            option = (metric, THRESHOLDS[metric])
            params = T.params_of(option)
            for occupied in (0, 50, 128):
                with step_limit(60, 'launch alone, N = {}, {}, {} slots'.format(N, metric, occupied)):
                    entry = T.track_rows_np(grid(128, occupied, 1)[None], option)[3] if occupied else T.empty_state()
                    state, nxt = T.state_tensor(entry, dev), T.state_tensor(None, dev)
                    med, low = median_us(lambda: hip.track(rows, state, params, state_out=nxt, out=out, ids=ids, hits=hits, workspace=work))
                    want = T.track_rows_np(host, option, entry)
                    same = ids.cpu().numpy().tolist() == want[1].tolist() and T.read_state(nxt)[0].tobytes() == want[3].tobytes()
                    records.append({'what': 'track launch', 'metric': metric, 'threshold': THRESHOLDS[metric], 'N': N, 'D': 100,
                                    'occupied_at_entry': occupied, 'occupied_at_exit': int((want[3]['id1'] != 0).sum()),
                                    'matched_rows': int((want[2] > 1).sum()), 'median_us': round(med, 2), 'min_us': round(low, 2),
                                    'us_per_frame': round(med / N, 2), 'equals_host_form': bool(same)})


def model_step(records, args):
    B, h, w = 8, 375, 1242
    option = ('dist', 2.0)
    with step_limit(600, 'building the model and its plan'):
        weights = W.synthetic_weights('resnet50', 1234)
        model = models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=option)
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        frames = (np.random.default_rng(0).integers(0, 2, size=(B, h, w, 3)) * 255).astype(np.uint8)
        call = [frames, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
        for _ in range(args.warmup):
            (rows, counts), _ = model.predict_poses_on_frames(*call)
            model.predict_tracks_on_frames(*call)
    for r in range(args.rounds):
        for name, run in (('predict_poses_on_frames', model.predict_poses_on_frames), ('predict_tracks_on_frames', model.predict_tracks_on_frames)):
            with step_limit(300, '{} round {}'.format(name, r)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run(*call)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1000.0 / args.steps
                records.append({'what': 'model call', 'call': name, 'round': r, 'B': B, 'frame': [h, w], 'dtype': args.dtype, 'track': list(option),
                                'ms_per_call': round(ms, 3), 'images_per_s': round(B * 1000.0 / ms, 1), 'rows': int(counts.sum())})
    state = model.track_state()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        T.track_rows_np(rows, option, state)
    ms = (time.perf_counter() - t0) * 1000.0 / args.steps
    records.append({'what': 'track_rows_np', 'B': B, 'rows': int(counts.sum()), 'occupied_at_entry': int((state['id1'] != 0).sum()),
                    'track': list(option), 'ms_per_call': round(ms, 3), 'ms_per_frame': round(ms / B, 3)})


def tables(records):
    out = ['| launch | metric | N | slots at entry | slots at exit | median us | min us | us per frame | == host form |', '|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'track launch':
            out.append('| gpp_track_f64 | {metric} | {N} | {occupied_at_entry} | {occupied_at_exit} | {median_us} | {min_us} | {us_per_frame} | '
                       '{equals_host_form} |'.format(**r))
    out += ['', '| call, B = 8 | round | ms per call | images/s | rows |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'model call':
            out.append('| {call} | {round} | {ms_per_call} | {images_per_s} | {rows} |'.format(**r))
    for r in records:
        if r['what'] == 'track_rows_np':
            out += ['', 'track_rows_np on the rows of one such call ({rows} rows, {occupied_at_entry} slots at entry): {ms_per_call} ms per call, '
                    '{ms_per_frame} ms per frame'.format(**r)]
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track'))
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    args = ap.parse_args()
    os.environ.setdefault('GPP_AUTOTUNE', '0')
    hip.require_device()
    os.makedirs(args.out, exist_ok=True)
    records = []
    launches_alone(records)
    model_step(records, args)
    with open(os.path.join(args.out, 'bench_track.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    with open(os.path.join(args.out, 'launch_tables.md'), 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
