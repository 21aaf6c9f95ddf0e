#!/usr/bin/env python3
"""
Measures utils.eval.evaluate on one GPU, in ONE process: a directory of `--images` generated PNG frames of the four KITTI sizes (labels
made from the model's own detections: copies, shifted copies, copies in another bin), read by KittiGenerator, resnet50, the 100-plane
database:

  (a) evaluate(device=True, batch_size=B)     raw frames up, preprocessing + resize + matching on the device (csrc/eval.hip)
  (b) evaluate(batch_size=B)                  float32 conversion + NumPy resize, eight arrays back, matching in Python

Both read and decode the same PNG files.  (a) and (b) alternate `--rounds` times in the same process on the same box (boxes differ by
several percent: numbers of two runs cannot be compared); their results must be equal (==).  Also: HIP events around the match launch
alone.  Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).
Writes <out>/bench_eval.jsonl; <out> defaults to profiles/eval.

    python tools/bench_eval.py [--out DIR] [--images 32] [--batch 8] [--rounds 3] [--dtype f16x3]
"""
import argparse
import contextlib
import io
import json
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

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.models import weights as W  # noqa: E402
from keras_retinanet_3D.preprocessing.kitti import KittiGenerator  # noqa: E402
from keras_retinanet_3D.utils import eval as gpp_eval  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402
from keras_retinanet_3D.utils.image import compute_resize_scale  # noqa: E402

KITTI_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_eval: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def labels_from_rows(rows):
    """ label rows (n, 17) from one image's detection rows (utils.eval._image_rows): by turns a copy, a copy shifted by a fifth of its
    width, one shifted by half, and a copy in the next orientation bin """
    out = []
    for j, r in enumerate(rows[:16]):
        box, rest, label, orientation = r[:4].copy(), r[4:15].copy(), r[-1], r[-2]
        if j % 4 in (1, 2):
            box[[0, 2]] += (0.2 if j % 4 == 1 else 0.5) * (box[2] - box[0])
            rest += 1.5
        if j % 4 == 3:
            orientation = (orientation + 1) % 4
        out.append(np.concatenate([box, rest, [label, orientation]]))
    return np.asarray(out, np.float64).reshape(-1, 17)


def write_dataset(base, model, n_images, batch):
    """ <base>/val/{images,labels,calibs} + the plane database; returns the number of labels """
    import scipy.io
    from PIL import Image
    planes = synthetic.load_plane_database('100')
    P2 = synthetic.KITTI_LIKE_P2
    for d in ('images', 'labels', 'calibs'):
        os.makedirs(os.path.join(base, 'val', d))
    scipy.io.savemat(os.path.join(base, 'road_planes_database.mat'), {'road_planes_database': planes})
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    n_labels = 0
    for first in range(0, n_images, batch):          # (the batch of the measurement: one plan serves everything)
        ids = list(range(first, min(first + batch, n_images)))
        frames = [(np.random.default_rng(100 + i).integers(0, 2, size=KITTI_SHAPES[i % 4] + (3,)) * 255).astype(np.uint8) for i in ids]
        P_inv = np.stack([synthetic.synthetic_calibration(compute_resize_scale(f.shape))[1] for f in frames])
        outputs, scales = model.predict_on_frames(frames, P_inv, np.tile(planes[None], (len(ids), 1, 1)))
        for k, i in enumerate(ids):
            Image.fromarray(frames[k][:, :, ::-1]).save(os.path.join(base, 'val', 'images', '%06d.png' % i))
            with open(os.path.join(base, 'val', 'calibs', '%06d.txt' % i), 'w') as f:
                f.write(calib)
            rows = labels_from_rows(gpp_eval._image_rows(outputs, k, float(scales[k]), 0.05, 100))
            n_labels += len(rows)
            with open(os.path.join(base, 'val', 'labels', '%06d.txt' % i), 'w') as f:
                f.write(''.join('Car 0 0 0 ' + ' '.join(repr(float(v)) for v in r[:15]) + ' %d\n' % int(r[16]) for r in rows))
    return n_labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval'))
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records = []

    def note(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def quiet(**kw):
        with contextlib.redirect_stdout(io.StringIO()):          # (evaluate prints its progress)
            return gpp_eval.evaluate(gen, model, batch_size=args.batch, **kw)

    with tempfile.TemporaryDirectory() as base:
        with step_limit(420, 'model, plans and the dataset'):
            model = models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype=args.dtype)
            n_labels = write_dataset(base, model, args.images, args.batch)
            gen = KittiGenerator(base, subset='val')
            want = quiet()
            got = quiet(device=True)
            hits = [(label, float(ap_), float(n)) for label, (ap_, n) in sorted(got[0].items())]
            note({'what': 'setup', 'images': gen.size(), 'batch': args.batch, 'dtype': args.dtype, 'labels': n_labels, 'device_equals_host': bool(got == want),
                  'average_precisions': hits, 'keypoint_error': float(got[1]), 'plans': len(model._plans), 'range_fallbacks': int(model.range_fallbacks),
                  'library': hip.lib().gpp_version().decode()})

        for r in range(args.rounds):
            for name, kw in (('device', {'device': True}), ('host', {})):
                with step_limit(300, '{} round {}'.format(name, r + 1)):
                    t0 = time.perf_counter()
                    quiet(**kw)
                    dt = time.perf_counter() - t0
                note({'what': 'evaluate', 'path': name, 'round': r + 1, 'seconds': round(dt, 4), 'images_per_s': round(gen.size() / dt, 2)})

        with step_limit(120, 'reading the frames alone'):
            t0 = time.perf_counter()
            for i in range(gen.size()):
                gen.load_image(i)
            dt = time.perf_counter() - t0
            note({'what': 'load_image_alone', 'seconds': round(dt, 4), 'images_per_s': round(gen.size() / dt, 2)})

        with step_limit(120, 'the match launch alone'):
            B = args.batch
            plan = model._last_plan
            outs = model.outputs(plan)
            dev = model.device
            anns = [gen.load_annotations(i)[0] for i in range(B)]
            A = max(len(a) for a in anns)
            padded = np.zeros((B, A, 17))
            for b, a in enumerate(anns):
                padded[b, :len(a)] = a
            ann_d = torch.as_tensor(padded).to(dev)
            cnt_d = torch.as_tensor(np.asarray([len(a) for a in anns], np.int32)).to(dev)
            scales_d = torch.full((B,), 1333.0 / 1242.0, dtype=torch.float32, device=dev)
            us = []
            for it in range(120):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                hip.eval_match(outs[0], outs[1], outs[2], outs[3], outs[4], scales_d, ann_d, cnt_d, 1, 0.05, 100, 0.5)
                e[1].record()
                e[1].synchronize()
                if it >= 20:
                    us.append(e[0].elapsed_time(e[1]) * 1e3)          # (includes the allocation of the three result tensors)
            note({'what': 'launch_alone', 'B': B, 'D': int(outs[2].shape[1]), 'A': A, 'median_us': round(statistics.median(us), 2), 'min_us': round(min(us), 2),
                  'launches': len(us)})

    with open(os.path.join(args.out, 'bench_eval.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    if not records[0]['device_equals_host']:
        sys.exit('bench_eval: evaluate(device=True) != evaluate()')


if __name__ == '__main__':
    main()
