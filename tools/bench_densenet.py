"""
DenseNet-121/169/201 throughput (images/s, B = 8, 402x1333, dtype f16x3 and f32) and the cost of the pre-activation 1x1 conv
(gpp_conv2d_preact) against the plain 1x1 conv (gpp_conv2d_igemm) at the same shapes.  One JSON line per measurement.
    python tools/bench_densenet.py [--backbones densenet121,...] [--dtypes f16x3,f32] [--steps 10] [--batch 8]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.layers import conv as C  # noqa: E402
from keras_retinanet_3D.models import weights as W  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402


def step_rate(backbone, dtype, B, H, Wd, steps):
    model = models.load_model('synthetic:1234', backbone_name=backbone, dtype=dtype)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    img = np.random.default_rng(0).integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - 120.0
    plan = model.stage_inputs([img, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))])
    for _ in range(3):
        model.run_plan(plan)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        model.run_plan(plan)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / steps
    return {'backbone': backbone, 'dtype': dtype, 'batch': B, 'hw': [H, Wd], 'images_per_s': round(B / dt, 1), 'ms_per_step': round(dt * 1e3, 2),
            'anchors_per_image': plan.n_anchors, 'conv_launches': sum(1 for op in plan.ops if op[0] in (3, 32))}


def time_us(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def preact_vs_plain(dtype, B, cin, cout, h, w):
    """ one 1x1 layer, both forms, each with its best tile """
    dev = torch.device('cuda')
    x = torch.randn((B, h, w, cin), device=dev)
    out = torch.empty((B, h, w, cout), device=dev)
    k = (np.random.default_rng(0).standard_normal((1, 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    wt, bias = C.pack_weight(k, dtype, dev), torch.zeros(cout, device=dev)
    s, t = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    osc = C.out_scale_of(k, dev) if dtype == 'f16x3' else None          # (alive as long as the descriptor that holds its address)
    d = C.conv_desc([C.FMap(x, B, h, w, cin)], [C.FMap(out, B, h, w, cout)], wt, bias, 1, 1, cin, cout, relu=True, dtype=dtype, out_scale=osc)
    best = ctypes.c_float(0.0)
    hip.check(hip.lib().gpp_conv2d_preact_autotune(ctypes.byref(d), ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(t.data_ptr()), 8,
                                                   hip.stream_ptr(), ctypes.byref(best)), 'preact autotune')
    pre_tile = int(d.tile_hint)
    pre = time_us(lambda: hip.lib().gpp_conv2d_preact(ctypes.byref(d), ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(t.data_ptr()), hip.stream_ptr()))
    d.tile_hint = 0
    hip.check(hip.lib().gpp_conv2d_autotune(ctypes.byref(d), 8, hip.stream_ptr(), ctypes.byref(best)), 'autotune')
    plain = time_us(lambda: hip.lib().gpp_conv2d_igemm(ctypes.byref(d), hip.stream_ptr()))
    n_cols = -(-cout // (pre_tile % 1000 or 128)) * (pre_tile % 1000 or 128)
    return {'layer': '1x1 {} -> {} at {}x{}x{}'.format(cin, cout, B, h, w), 'dtype': dtype, 'preact_us': round(pre, 1), 'plain_us': round(plain, 1),
            'preact_tile': pre_tile, 'plain_tile': int(d.tile_hint), 'ratio': round(pre / plain, 3),
            'dead_column_share': round(1.0 - cout / n_cols, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--backbones', default='densenet121,densenet169,densenet201')
    ap.add_argument('--dtypes', default='f16x3,f32')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-layers', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if not a.no_layers:
        # densenet121 at B = 8, 402x1333: a _1_conv early and late in each block, and a transition
        for dtype in a.dtypes.split(','):
            for cin, cout, h, w in ((64, 128, 101, 334), (224, 128, 101, 334), (128, 128, 50, 167), (480, 128, 50, 167), (992, 128, 25, 83),
                                    (512, 256, 50, 167), (1024, 512, 25, 83), (992, 128, 12, 41)):
                print(json.dumps(preact_vs_plain(dtype, a.batch, cin, cout, h, w)), flush=True)
    for backbone in a.backbones.split(','):
        for dtype in a.dtypes.split(','):
            print(json.dumps(step_rate(backbone, dtype, a.batch, 402, 1333, a.steps)), flush=True)


if __name__ == '__main__':
    main()
