#!/usr/bin/env python3
"""
Measures the device pose stage (csrc/pose.hip, RetinaNet3D(pose=True)) on one GPU, in ONE process:

  1. the pose launch alone at B = 1, 8, 16 (100 detections per image, the rows of a committed fixture): HIP events around each
     launch, median of 200;
  2. at B = 8, resnet50, the 1k plane database, 402 x 1333: images/s of "predict + post-processing up to the KITTI text in memory" for
        (a) the host path:   predict_on_batch -> select_detections -> recover_pose -> kitti_lines, per image
        (b) the device path: predict_poses_on_batch -> kitti_lines_from_rows, per image
     (a) and (b) alternate three times in the same process on the same box (boxes differ by several percent: numbers of two runs cannot
     be compared), the way tools/ab_bench.sh alternates two builds;
  3. the deviation of the device rows and of the host path from the float64 oracle (tests/pose_oracle.py) on the committed fixtures.

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_pose.jsonl (one JSON record per measurement) and <out>/README.md (the tables); <out> defaults to profiles/pose.

    python tools/bench_pose.py [--out DIR] [--steps 30] [--warmup 5] [--rounds 3] [--dtype f16x3]
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
from keras_retinanet_3D.utils import gpp_utils, synthetic  # noqa: E402

MEAN = np.array([103.939, 116.779, 123.68], np.float32)
SCALE, SHAPE = 402.0 / 375.0, (375, 1242, 3)


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('bench_pose: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def launch_alone(records):
    import pose_oracle as O
    outs, _, _ = O.fixture_outputs('fullsize_resnet50_1k_f64.npz')
    dev = torch.device('cuda', torch.cuda.current_device())
    for B in (1, 8, 16):
        with step_limit(60, 'pose launch alone, B = {}'.format(B)):
            t = [torch.as_tensor(np.ascontiguousarray(o[:B])).to(dev) for o in outs]
            info = torch.tensor([[SCALE, SHAPE[0], SHAPE[1]]] * B, dtype=torch.float32, device=dev)
            rows = torch.empty((B, 100, hip.GPP_POSE_COLS), dtype=torch.float32, device=dev)
            counts = torch.zeros((B,), dtype=torch.int32, device=dev)
            args = [hip.ptr(t[0]), hip.ptr(t[1]), hip.ptr(t[2]), hip.ptr(t[3]), hip.ptr(t[4]), hip.ptr(t[5]), hip.ptr(t[7]), hip.ptr(info),
                    B, 100, 0.05, hip.ptr(rows), hip.ptr(counts)]
            lib = hip.lib()
            for _ in range(20):
                hip.check(lib.gpp_pose_f32(*(args + [hip.stream_ptr()])), 'gpp_pose_f32')
            torch.cuda.synchronize()
            us = []
            for _ in range(200):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.check(lib.gpp_pose_f32(*(args + [hip.stream_ptr()])), 'gpp_pose_f32')
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            assert int(counts.sum().item()) == 100 * B
            rec = {'what': 'pose_launch_alone', 'B': B, 'detections': 100 * B, 'median_us': round(statistics.median(us), 2),
                   'min_us': round(min(us), 2), 'p90_us': round(sorted(us)[179], 2), 'launches': 200}
            records.append(rec)
            print(json.dumps(rec))


def host_leg(model, inputs, steps):
    t0 = time.perf_counter()
    chars = 0
    for _ in range(steps):
        outs = model.predict_on_batch(inputs)
        for k in range(inputs[0].shape[0]):
            det = gpp_utils.recover_pose(gpp_utils.select_detections(outs, SCALE, image_index=k))
            chars += len(''.join(gpp_utils.kitti_lines(det, SHAPE)))
    return time.perf_counter() - t0, chars


def device_leg(model, inputs, steps):
    t0 = time.perf_counter()
    chars = 0
    for _ in range(steps):
        rows, counts = model.predict_poses_on_batch(inputs, SCALE, SHAPE)
        for k in range(inputs[0].shape[0]):
            chars += len(gpp_utils.kitti_lines_from_rows(rows[k], counts[k]))
    return time.perf_counter() - t0, chars


def end_to_end(records, args):
    B, H, Wd = 8, 402, 1333
    with step_limit(420, 'models and plans'):
        weights = W.synthetic_weights('resnet50', 1234)
        plain = models.load_model(weights, backbone_name='resnet50', dtype=args.dtype)
        posed = models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True)
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration(SCALE)
        rng = np.random.default_rng(0)              # binary noise: about 100 detections above the threshold per image
        frames = (rng.integers(0, 2, size=(B, H, Wd, 3)) * 255).astype(np.float32) - MEAN
        inputs = [frames, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
        host_leg(plain, inputs, args.warmup)
        device_leg(posed, inputs, args.warmup)
        detections = int((plain.predict_on_batch(inputs)[2] > 0.05).sum())
    for r in range(args.rounds):
        for name, leg, model in (('host_path', host_leg, plain), ('device_path', device_leg, posed)):
            with step_limit(180, '{} round {}'.format(name, r + 1)):
                dt, chars = leg(model, inputs, args.steps)
            rec = {'what': 'end_to_end', 'path': name, 'round': r + 1, 'B': B, 'H': H, 'W': Wd, 'dtype': args.dtype, 'planes': '1k',
                   'steps': args.steps, 'detections_per_batch': detections, 'kitti_chars': chars,
                   'images_per_s': round(B * args.steps / dt, 1), 'ms_per_step': round(1e3 * dt / args.steps, 3)}
            records.append(rec)
            print(json.dumps(rec))


def deviations(records):
    import pose_oracle as O
    worst, differ = {}, {'device': 0, 'host_path': 0}
    n_rows = 0
    with step_limit(300, 'deviations on the fixtures'):
        for fx in O.FIXTURES:
            outs, scales, shapes = O.fixture_outputs(fx)
            want, counts = O.pose_rows(outs, scales, shapes)
            host = O.host_rows(outs, scales, shapes)
            rows, _ = gpp_utils.recover_pose_device(outs, scales, shapes)
            valid = want[..., O.SCORE] > 0
            n_rows += int(valid.sum())
            for name, cols, angular in O.GROUPS:
                w = worst.setdefault(name, [0.0, 0.0])
                w[0] = max(w[0], float(O.deviation(rows, want, cols, angular)[valid].max()))
                w[1] = max(w[1], float(O.deviation(host, want, cols, angular)[valid].max()))
            for b in range(want.shape[0]):
                for r_w, r_h, r_d in zip(want[b, :counts[b]], host[b, :counts[b]], rows[b, :counts[b]]):
                    for a, h, d in zip(O.kitti_fields(r_w), O.kitti_fields(r_h), O.kitti_fields(r_d)):
                        differ['device'] += ('%.2f' % a) != ('%.2f' % d)
                        differ['host_path'] += ('%.2f' % a) != ('%.2f' % h)
    rec = {'what': 'deviation_from_float64_oracle', 'rows': n_rows, 'text_fields': 13 * n_rows, 'text_fields_differing': differ,
           'max_abs_deviation': {k: {'device': v[0], 'host_path': v[1]} for k, v in worst.items()}}
    records.append(rec)
    print(json.dumps(rec))


def write_readme(path, records, args):
    alone = [r for r in records if r['what'] == 'pose_launch_alone']
    e2e = [r for r in records if r['what'] == 'end_to_end']
    dev = [r for r in records if r['what'] == 'deviation_from_float64_oracle']
    lines = ['# Device pose stage: measurements', '',
             'Written by `tools/bench_pose.py` ({}; one process, one MI355X; library {}).'.format(
                 time.strftime('%Y-%m-%d'), hip.lib().gpp_version().decode()),
             'Raw records: `bench_pose.jsonl`.', '']
    if alone:
        lines += ['## The pose launch alone', '', 'HIP events around one `gpp_pose_f32` launch, 200 launches, 100 detections per image.', '',
                  '| B | median us | min us | p90 us |', '|---|---|---|---|']
        lines += ['| {B} | {median_us} | {min_us} | {p90_us} |'.format(**r) for r in alone]
        lines += ['']
    if e2e:
        lines += ['## Predict + post-processing up to the KITTI text in memory', '',
                  'B = 8, resnet50, {}, 1k planes, 402 x 1333, {} steps per leg after {} warm-up steps, {} detections above 0.05 per batch;'.format(
                      args.dtype, args.steps, args.warmup, e2e[0]['detections_per_batch']),
                  'host path = `predict_on_batch` -> `select_detections` -> `recover_pose` -> `kitti_lines` (the code of the parent commit, unchanged),',
                  'device path = `predict_poses_on_batch` -> `kitti_lines_from_rows`.  The legs alternate in one process on one box.', '',
                  '| round | host path images/s | device path images/s | ratio |', '|---|---|---|---|']
        for r in sorted(set(x['round'] for x in e2e)):
            a = [x for x in e2e if x['round'] == r and x['path'] == 'host_path'][0]['images_per_s']
            b = [x for x in e2e if x['round'] == r and x['path'] == 'device_path'][0]['images_per_s']
            lines.append('| {} | {} | {} | {:.3f} |'.format(r, a, b, b / a))
        ha = [x['images_per_s'] for x in e2e if x['path'] == 'host_path']
        hb = [x['images_per_s'] for x in e2e if x['path'] == 'device_path']
        lines += ['', 'Spread over the rounds: host path {} - {}, device path {} - {} images/s.'.format(min(ha), max(ha), min(hb), max(hb)), '']
    if dev:
        d = dev[0]
        lines += ['## Deviation from the float64 oracle', '',
                  'Largest absolute deviation from `tests/pose_oracle.py` over the {} rows of the three resnet50 fixtures and the two harness'.format(d['rows']),
                  'goldens (angles modulo 2 pi); the bar of `tests/test_pose_gpu.py` is max(host path, 4 float32 ulp of the oracle value).', '',
                  '| field group | device rows | host path |', '|---|---|---|']
        lines += ['| {} | {:.3e} | {:.3e} |'.format(k, v['device'], v['host_path']) for k, v in d['max_abs_deviation'].items()]
        lines += ['', 'The largest figures (dimensions, locations, KITTI height) belong to detections of the synthetic weights that lie tens of kilometres away:',
                  'they are half a float32 ulp of the value there.',
                  '', 'KITTI text (`%.2f`), fields differing from the oracle\'s text out of {}: device rows {}, host path {}.'.format(
            d['text_fields'], d['text_fields_differing']['device'], d['text_fields_differing']['host_path']), '']
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose'))
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    if 'GPP_TUNE_CACHE' not in os.environ:          # both models run the tiles the first one timed: the legs differ by the pose stage only
        import tempfile
        os.environ['GPP_TUNE_CACHE'] = os.path.join(tempfile.mkdtemp(prefix='gpp_tiles_'), 'tile_choices.json')
    records = []
    launch_alone(records)
    deviations(records)
    end_to_end(records, args)
    with open(os.path.join(args.out, 'bench_pose.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    write_readme(os.path.join(args.out, 'README.md'), records, args)


if __name__ == '__main__':
    main()
