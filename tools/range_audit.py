#!/usr/bin/env python3
"""
The range audit of dtype='f16x3' (models.load_model(..., range_audit=True)) from the command line.

    python tools/range_audit.py --backbone resnet50 --weights synthetic:1234 --batch 8 --size 402x1333 [--json FILE]
        loads the model with range_audit=True, runs seeded noise frames through it and prints the report: one line per audited map,
        smallest maximum first (name, readers, channels, live channels, the map's largest |x|, the smallest / median channel maximum,
        channels below 2^-9, bits the largest value keeps in an IEEE-half pair, FLAGGED), then the operands a pass over HBM cannot
        see.  --weights takes what load_model takes (synthetic:<seed>[:trained], .npz, .h5).  --json appends one JSON line.

    python tools/range_audit.py --bench [--out DIR]
        in ONE process on one GPU (numbers of two boxes cannot be compared):
        1. gpp_channel_absmax alone on the largest map of the B = 8 plan at 402 x 1333 (res2: 8 x 101 x 334 x 256, float32 rows and
           pre-split rows) and on a tower map (8 x 11438 x 256 pre-split), beside a plain read-only pass over the same bytes (a
           float32 sum): HIP events around every launch, median of 40, once on one buffer (what the 256 MiB Infinity Cache keeps of
           it stays) and once rotating over four buffers (cold);
        2. the audit plan against the ordinary plan of the same model at B = 8, 402 x 1333, alternating three times: ms per step.
        Writes <out>/bench_range_audit.jsonl; <out> defaults to profiles/range_audit.
Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).
"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.models import retinanet as R  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402

MEAN = np.array([103.939, 116.779, 123.68], np.float32)


class step_limit(object):
    """ with step_limit(seconds, what): ... -- the process ends if the block runs longer """

    def __init__(self, seconds, what):
        self.seconds, self.what = int(seconds), what

    def _expired(self, *_):
        sys.stderr.write('range_audit: step "{}" ran longer than {} s: stopping here\n'.format(self.what, self.seconds))
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._expired)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def noise_inputs(B, H, Wd, planes='1k', seed=0):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - MEAN
    db = synthetic.load_plane_database(planes).astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return [img, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(db[None], (B, 1, 1))]


def print_report(report, unobserved):
    print('{:<30} {:>5} {:>5} {:>11} {:>11} {:>11} {:>6} {:>4}  readers'.format('map', 'chan', 'live', 'absmax', 'min live', 'median', '<2^-9', 'bits'))
    for r in sorted(report, key=lambda r: (r['absmax'] != r['absmax'], r['absmax'])):
        fmt = lambda v: '-' if v is None else '{:.4g}'.format(v)  # noqa: E731
        print('{:<30} {:>5} {:>5} {:>11} {:>11} {:>11} {:>6} {:>4}  {}{}'.format(
            r['name'][:30], r['channels'], r['live'], fmt(r['absmax']), fmt(r['absmax_min_live']), fmt(r['absmax_median_live']),
            r['small_channels'], '-' if r['bits'] is None else r['bits'], ', '.join(r['consumers']), '   FLAGGED' if r['flagged'] else ''))
    if unobserved:
        print('not observable by a pass over HBM ({}): {} ...'.format(len(unobserved), '; '.join('{} ({})'.format(u['name'], u['reason']) for u in unobserved[:2])))


def report(args):
    H, Wd = (int(v) for v in args.size.lower().split('x'))
    with step_limit(600, 'report'):
        model = models.load_model(args.weights, backbone_name=args.backbone, dtype='f16x3', range_audit=True, on_range_event='ignore')
        model.predict_on_batch(noise_inputs(args.batch, H, Wd))
        rep, unseen = model.last_range_audit, model.range_audit_unobserved()
    print_report(rep, unseen)
    smallest = min(rep, key=lambda r: (r['absmax'] != r['absmax'], r['absmax']))
    line = {'what': 'report', 'backbone': args.backbone, 'weights': args.weights, 'batch': args.batch, 'size': [H, Wd], 'maps': len(rep),
            'flagged': [r['name'] for r in rep if r['flagged']], 'smallest_map': smallest['name'], 'smallest_map_absmax': smallest['absmax'],
            'smallest_map_over_threshold': smallest['absmax'] / R.RANGE_AUDIT_THRESHOLD,
            'maps_with_small_channels': sum(1 for r in rep if r['small_channels']), 'small_channels': sum(r['small_channels'] for r in rep),
            'live_channels': sum(r['live'] for r in rep), 'channels': sum(r['channels'] for r in rep), 'unobserved': len(unseen)}
    print(json.dumps(line))
    if args.json:
        with open(args.json, 'a') as f:
            f.write(json.dumps(line) + '\n')


def time_launches(fn, n_buffers, iters=40, warmup=4):
    """ median ms of fn(k) (k: which buffer) over `iters` launches, an event pair around each """
    for k in range(warmup):
        fn(k % n_buffers)
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for k, (e0, e1) in enumerate(pairs):
        e0.record()
        fn(k % n_buffers)
        e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs)


def bench_kernel(out, name, M, C, layout):
    dev = torch.device('cuda')
    nbytes = M * C * 4
    bufs = [torch.randn((M, C), dtype=torch.float32, device=dev) for _ in range(4)]
    if layout != hip.GPP_ABSMAX_F32:           # any bytes are valid halves; keep them finite numbers of ordinary size
        bufs = [(b.half().view(torch.float32).repeat(1, 2)).contiguous() for b in bufs]
    table = torch.zeros((C,), dtype=torch.int32, device=dev)
    for mode, n in (('one buffer', 1), ('four buffers in turn', 4)):
        ms = time_launches(lambda k: hip.channel_absmax(bufs[k], M, C, C, 0, layout, table), n)
        ref = time_launches(lambda k: bufs[k].sum(), n)
        line = {'what': 'kernel', 'map': name, 'M': M, 'C': C, 'layout': {1: 'f32', 2: 'split_f16', 3: 'split_bf16'}[layout], 'bytes': nbytes, 'buffers': mode,
                'absmax_ms': round(ms, 4), 'absmax_GBps': round(nbytes / ms / 1e6, 1), 'read_pass_ms': round(ref, 4), 'read_pass_GBps': round(nbytes / ref / 1e6, 1),
                'ratio': round(ref / ms, 3)}
        print(json.dumps(line))
        out.write(json.dumps(line) + '\n')
    del bufs


def bench(args):
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'bench_range_audit.jsonl'), 'w') as out:
        with step_limit(240, 'kernel alone'):
            bench_kernel(out, 'res2 block output, float32 rows', 8 * 101 * 334, 256, hip.GPP_ABSMAX_F32)
            bench_kernel(out, 'res2 block output, pre-split', 8 * 101 * 334, 256, hip.GPP_ABSMAX_SPLIT_F16)
            bench_kernel(out, 'classification tower map, pre-split', 8 * 11438, 256, hip.GPP_ABSMAX_SPLIT_F16)
        with step_limit(600, 'plans'):
            B, H, Wd = 8, 402, 1333
            x = noise_inputs(B, H, Wd)
            plain = models.load_model(args.weights, backbone_name=args.backbone, dtype='f16x3')
            audit = models.load_model(args.weights, backbone_name=args.backbone, dtype='f16x3', range_audit=True)
            unfused = None
            os.environ['GPP_FUSE_BLOCK'], os.environ['GPP_FUSE_TAIL'] = '', ''
            try:                                # the ordinary plan with the separate launches an audit plan uses: what the unfusing alone costs
                unfused = models.load_model(args.weights, backbone_name=args.backbone, dtype='f16x3')
                plans = {'unfused': (unfused, unfused.stage_inputs(x))}
            finally:
                del os.environ['GPP_FUSE_BLOCK'], os.environ['GPP_FUSE_TAIL']
            plans.update({'ordinary': (plain, plain.stage_inputs(x)), 'audit': (audit, audit.stage_inputs(x))})
            torch.cuda.synchronize()
            times = {k: [] for k in plans}
            for _ in range(args.rounds):
                for k, (m, p) in plans.items():
                    for _ in range(args.warmup):
                        m.run_plan(p)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        m.run_plan(p)
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) / args.steps)
            pa = plans['audit'][1]
            launches = sum(1 for op in pa.ops if op[0] == R.OP_ABSMAX)
            audited = sum(op[2].M * op[2].C * 4 for op in pa.ops if op[0] == R.OP_ABSMAX)
            line = {'what': 'plan', 'backbone': args.backbone, 'weights': args.weights, 'batch': B, 'size': [H, Wd], 'steps': args.steps, 'rounds': args.rounds,
                    'ms_per_step': {k: [round(v, 4) for v in t] for k, t in times.items()},
                    'median_ms_per_step': {k: round(statistics.median(t), 4) for k, t in times.items()},
                    'absmax_launches': launches, 'audited_bytes': audited, 'ops': {k: len(p.ops) for k, (_, p) in plans.items()}}
            print(json.dumps(line))
            out.write(json.dumps(line) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--backbone', default='resnet50')
    ap.add_argument('--weights', default='synthetic:1234')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', default='402x1333')
    ap.add_argument('--json', default=None, help='append the summary line of the report to this file')
    ap.add_argument('--bench', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'range_audit'))
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    hip.require_device()
    if args.bench:
        bench(args)
    else:
        report(args)


if __name__ == '__main__':
    main()
