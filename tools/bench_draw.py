#!/usr/bin/env python3
"""
Measures the --save-images composites (csrc/draw.hip, RetinaNet3D.predict_composites_on_frames) on one GPU, in ONE process, at B = 8 on the
four KITTI frame sizes (a ragged list), resnet50, the 1k plane database:

  (a) predict_composites_on_frames                              pictures rendered on the device, one more copy to the host
  (b) predict_poses_on_frames, then utils.visualization.composite_from_rows per image      pictures rendered on the host
  (c) predict_poses_on_frames alone                             what both are paid on top of
  (d) PNG encoding of the eight pictures (utils.visualization.write_png into memory), timed separately: the CLI pays it on either path

(a), (b) and (c) alternate `--rounds` times in the same process on the same box (boxes differ by several percent: numbers of two runs
cannot be compared).  Also: HIP events around the two draw launches alone.  Every GPU step runs under a time limit of its own (SIGALRM:
the process ends there, nothing more is started).  Writes <out>/bench_draw.jsonl; <out> defaults to profiles/draw.

    python tools/bench_draw.py [--out DIR] [--steps 20] [--warmup 3] [--rounds 3] [--dtype f16x3] [--threshold 0.05]
"""
import argparse
import io
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
from keras_retinanet_3D.utils import visualization as vis  # noqa: E402
from keras_retinanet_3D.utils.image import compute_resize_scale  # noqa: E402

KITTI_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_draw: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'draw'))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    ap.add_argument('--threshold', type=float, default=0.05, help='synthetic scores rarely pass the CLI default of 0.4')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records = []

    def note(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    B = 8
    shapes = [KITTI_SHAPES[k % 4] for k in range(B)]
    with step_limit(420, 'model and plan'):
        model = models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype=args.dtype, pose=True)
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        P2 = synthetic.KITTI_LIKE_P2
        frames = [(np.random.default_rng(k).integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8) for k, (h, w) in enumerate(shapes)]
        P_inv = np.stack([np.linalg.pinv(np.diag([s, s, 1.0]).dot(P2)) for s in (compute_resize_scale((h, w, 3)) for h, w in shapes)]).astype(np.float32)
        P_raw = np.stack([P2] * B)

        def device_leg():
            return model.predict_composites_on_frames(frames, P_inv, planes, P_raw, args.threshold)

        def host_leg():
            (rows, counts), scale = model.predict_poses_on_frames(frames, P_inv, planes)
            return (rows, counts), scale, [vis.composite_from_rows(f, rows[b], counts[b], P_raw[b], args.threshold) for b, f in enumerate(frames)]

        def poses_leg():
            return model.predict_poses_on_frames(frames, P_inv, planes)

        for _ in range(args.warmup):
            (rows, counts), _, device_pictures = device_leg()
            _, _, host_pictures = host_leg()
            poses_leg()
        drawn = [int((rows[b, :counts[b], 12] > np.float32(args.threshold)).sum()) for b in range(B)]
        same = all(np.array_equal(a, b) for a, b in zip(device_pictures, host_pictures))
        note({'what': 'setup', 'B': B, 'shapes': shapes, 'dtype': args.dtype, 'threshold': args.threshold, 'detections_drawn': drawn,
              'device_equals_host': bool(same), 'picture_bytes': int(sum(p.nbytes for p in device_pictures)), 'library': hip.lib().gpp_version().decode()})

    for r in range(args.rounds):
        for name, leg in (('device_composites', device_leg), ('poses_then_host_renderer', host_leg), ('poses_alone', poses_leg)):
            with step_limit(240, '{} round {}'.format(name, r + 1)):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    leg()
                dt = time.perf_counter() - t0
            note({'what': 'end_to_end', 'path': name, 'round': r + 1, 'steps': args.steps, 'ms_per_step': round(1e3 * dt / args.steps, 3),
                  'images_per_s': round(B * args.steps / dt, 1)})

    with step_limit(120, 'draw launches alone'):
        dev = model.device
        rows_d = torch.as_tensor(rows).to(dev)
        P_d = torch.as_tensor(P_raw).to(dev)
        Hr, Wr = max(s[0] for s in shapes), max(s[1] for s in shapes)
        raw = np.zeros((B, Hr * Wr * 3), np.uint8)
        for b, f in enumerate(frames):
            raw[b, :f.size] = f.reshape(-1)
        frames_d = torch.as_tensor(raw).to(dev)
        hw = torch.as_tensor(np.asarray(shapes, dtype=np.int32)).to(dev)
        out = torch.empty((B, 2 * Hr * Wr * 3), dtype=torch.uint8, device=dev)
        status = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        prims, prim_counts = hip.draw_build(rows_d, P_d, args.threshold)
        us = {'build': [], 'raster': []}
        for it in range(120):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            prims, prim_counts = hip.draw_build(rows_d, P_d, args.threshold)
            e[1].record()
            hip.draw_raster(frames_d, hw, Hr, Wr, prims, prim_counts, out, status)
            e[2].record()
            e[2].synchronize()
            if it >= 20:
                us['build'].append(e[0].elapsed_time(e[1]) * 1e3)          # (includes the allocation of the table)
                us['raster'].append(e[1].elapsed_time(e[2]) * 1e3)
        for k, v in us.items():
            note({'what': 'launch_alone', 'stage': k, 'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'launches': len(v)})

    with step_limit(240, 'PNG encoding'):
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            size = 0
            for p in device_pictures:
                buf = io.BytesIO()
                vis.write_png(buf, p)
                size += buf.tell()
            t.append(time.perf_counter() - t0)
        note({'what': 'png_encoding', 'pictures': B, 'ms_per_batch': round(1e3 * statistics.median(t), 1), 'png_bytes': size})

    with open(os.path.join(args.out, 'bench_draw.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
