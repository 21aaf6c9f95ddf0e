#!/usr/bin/env python3
"""
Measures the cuboid NMS stage (csrc/cuboid_nms.hip, RetinaNet3D(pose=True, cuboid_nms=...)) on one GPU, in ONE process:

  1. the launch alone at B = 1, 8, 16 and D = 100, both metrics, for two scenes --
        sparse: 100 cars on a 10 x 10 grid, 12 m apart: no overlapping pair (the centre-distance gate skips every clipping);
        dense:  25 cars, each with three jittered duplicates: every detection overlaps three others --
     HIP events around each launch, median of 200; next to it, measured the same way, the pose launch (gpp_pose_f32, the rows of a
     committed fixture) and the polling launch (gpp_poll_f32, the 1k plane database) at the same B;
  2. at B = 8, resnet50, the 1k plane database, 402 x 1333 raw frames: ms per predict_poses_on_frames call with and without the stage
     (two models on the same weights), alternating three times in the same process on the same box (boxes differ by several percent:
     numbers of two runs cannot be compared).

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_cuboid_nms.jsonl (one JSON record per measurement) and <out>/launch_tables.md (the tables that <out>/README.md quotes); <out>
defaults to profiles/cuboid_nms.

    python tools/bench_cuboid_nms.py [--out DIR] [--steps 30] [--warmup 5] [--rounds 3] [--dtype f16x3] [--threshold 0.3]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.models import weights as W  # noqa: E402
from keras_retinanet_3D.utils import cuboid_nms, gpp_utils, synthetic  # noqa: E402

SCALE, SHAPE = 402.0 / 375.0, (375, 1242, 3)


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_cuboid_nms: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def scene(kind, seed):
    """ (100, 36) float32 rows: only the columns the stage reads are filled """
    rng = np.random.default_rng(seed)
    rows = np.zeros((100, 36), np.float32)
    rows[:, 12] = rng.permutation(np.linspace(0.06, 0.99, 100)).astype(np.float32)
    if kind == 'sparse':
        k = np.arange(100)
        x, z, ry = -54.0 + 12.0 * (k % 10), 8.0 + 12.0 * (k // 10), rng.uniform(-np.pi, np.pi, 100)
    else:
        c = np.arange(100) // 4
        x = -24.0 + 12.0 * (c % 5) + rng.normal(0.0, 0.2, 100)
        z = 8.0 + 12.0 * (c // 5) + rng.normal(0.0, 0.2, 100)
        ry = np.repeat(rng.uniform(-np.pi, np.pi, 25), 4) + rng.normal(0.0, 0.05, 100)
    rows[:, 16], rows[:, 17], rows[:, 18], rows[:, 30] = 1.5, 1.6, 4.0, 1.5
    rows[:, 19], rows[:, 20], rows[:, 21], rows[:, 31], rows[:, 32] = x, 1.65, z, 1.65, ry
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


def launches_alone(records, threshold):
    import pose_oracle as O
    dev = torch.device('cuda', torch.cuda.current_device())
    lib = hip.lib()
    outs, _, _ = O.fixture_outputs('fullsize_resnet50_1k_f64.npz')
    planes = torch.as_tensor(synthetic.load_plane_database('1k').astype(np.float32)).to(dev)
    _, P_inv = synthetic.synthetic_calibration()
    for B in (1, 8, 16):
        with step_limit(120, 'launches alone, B = {}'.format(B)):
            for kind in ('sparse', 'dense'):
                host = np.stack([scene(kind, 100 * B + b) for b in range(B)])
                src = torch.as_tensor(host).to(dev)
                out, counts, by = torch.empty_like(src), torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B, 100), dtype=torch.int32, device=dev)
                for code, metric in enumerate(cuboid_nms.METRICS):
                    med, low = median_us(lambda: hip.cuboid_nms(src, code, threshold, out=out, counts=counts, suppressor=by))
                    kept = counts.cpu().numpy()
                    want = cuboid_nms.suppress_batch_np(host, metric, threshold)[1]
                    records.append({'what': 'cuboid_nms launch', 'scene': kind, 'metric': metric, 'B': B, 'D': 100, 'threshold': threshold,
                                    'median_us': round(med, 2), 'min_us': round(low, 2), 'kept_per_image': float(kept.mean()), 'counts_equal_host_form': kept.tolist() == want.tolist()})
            reps = -(-B // outs[0].shape[0])
            t = [torch.as_tensor(np.ascontiguousarray(np.concatenate([o] * reps)[:B])).to(dev) for o in outs]
            info = torch.tensor([[SCALE, SHAPE[0], SHAPE[1]]] * B, dtype=torch.float32, device=dev)
            rows = torch.empty((B, 100, hip.GPP_POSE_COLS), dtype=torch.float32, device=dev)
            pc = torch.zeros((B,), dtype=torch.int32, device=dev)
            args = [hip.ptr(t[0]), hip.ptr(t[1]), hip.ptr(t[2]), hip.ptr(t[3]), hip.ptr(t[4]), hip.ptr(t[5]), hip.ptr(t[7]), hip.ptr(info),
                    B, 100, 0.05, hip.ptr(rows), hip.ptr(pc)]
            med, low = median_us(lambda: hip.check(lib.gpp_pose_f32(*(args + [hip.stream_ptr()])), 'gpp_pose_f32'))
            records.append({'what': 'pose launch', 'B': B, 'D': 100, 'median_us': round(med, 2), 'min_us': round(low, 2)})
            pinv = torch.as_tensor(np.tile(P_inv[None].astype(np.float32), (B, 1, 1))).to(dev)
            med, low = median_us(lambda: gpp_utils.fit_road_planes(t[0], t[1], t[4], pinv, planes))
            records.append({'what': 'polling launch (with its output allocation)', 'B': B, 'D': 100, 'planes': int(planes.shape[0]),
                            'median_us': round(med, 2), 'min_us': round(low, 2)})


def model_step(records, args):
    B, h, w = 8, 375, 1242
    with step_limit(600, 'building the two models and their plans'):
        weights = W.synthetic_weights('resnet50', 1234)
        plain = models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True)
        staged = models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, cuboid_nms=('bev', args.threshold))
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        rng = np.random.default_rng(0)
        frames = (rng.integers(0, 2, size=(B, h, w, 3)) * 255).astype(np.uint8)
        call = [frames, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
        for m in (plain, staged):
            for _ in range(args.warmup):
                (rows, counts), _ = m.predict_poses_on_frames(*call)
        kept = int(counts.sum())
        (rows0, counts0), _ = plain.predict_poses_on_frames(*call)
    for r in range(args.rounds):
        for name, m in (('without the stage', plain), ('with the stage', staged)):
            with step_limit(300, 'predict_poses_on_frames {} round {}'.format(name, r)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    m.predict_poses_on_frames(*call)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1000.0 / args.steps
                records.append({'what': 'predict_poses_on_frames', 'model': name, 'round': r, 'B': B, 'frame': [h, w], 'dtype': args.dtype,
                                'ms_per_call': round(ms, 3), 'images_per_s': round(B * 1000.0 / ms, 1),
                                'rows': int(counts0.sum()), 'rows_kept': kept if m is staged else int(counts0.sum())})


def tables(records):
    out = ['| launch | scene | metric | B | median us | min us | kept per image |', '|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'cuboid_nms launch':
            out.append('| gpp_cuboid_nms_f64 | {scene} | {metric} | {B} | {median_us} | {min_us} | {kept_per_image} |'.format(**r))
    for r in records:
        if r['what'].startswith(('pose launch', 'polling launch')):
            out.append('| {} | | | {} | {} | {} | |'.format(r['what'], r['B'], r['median_us'], r['min_us']))
    out += ['', '| predict_poses_on_frames, B = 8 | round | ms per call | images/s | rows | rows kept |', '|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'predict_poses_on_frames':
            out.append('| {model} | {round} | {ms_per_call} | {images_per_s} | {rows} | {rows_kept} |'.format(**r))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cuboid_nms'))
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    ap.add_argument('--threshold', type=float, default=0.3)
    args = ap.parse_args()
    os.environ.setdefault('GPP_AUTOTUNE', '0')
    hip.require_device()
    os.makedirs(args.out, exist_ok=True)
    records = []
    launches_alone(records, args.threshold)
    model_step(records, args)
    with open(os.path.join(args.out, 'bench_cuboid_nms.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    with open(os.path.join(args.out, 'launch_tables.md'), 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
