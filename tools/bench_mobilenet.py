"""
MobileNet throughput beside ResNet-50 in the same process (images/s at B = 8, 402x1333, dtype f16x3 and f32), the stem + backbone time
of both, every depthwise-separable block against its compulsory bytes (input + output + weights), and the fused block against the same
block run as depthwise-to-HBM plus a plain 1x1 convolution (a timing-only leg: no plan runs it).  One JSON line per measurement.
    python tools/bench_mobilenet.py [--backbone mobilenet224_1.0] [--dtypes f16x3,f32] [--steps 20] [--batch 8] [--out FILE]
Timing: device events around `steps` back-to-back launches after warm-up, the median of five such windows (tile choices come from the
model's own autotuner, made before anything is timed).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.layers import conv as C  # noqa: E402
from keras_retinanet_3D.layers import mobilenet as M  # noqa: E402
from keras_retinanet_3D.models import retinanet as R  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402


def time_us(fn, iters, windows=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    got = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        got.append(e0.elapsed_time(e1) * 1e3 / iters)
    return float(np.median(got))


def staged(backbone, dtype, B, H, Wd):
    model = models.load_model('synthetic:1234', backbone_name=backbone, dtype=dtype)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    img = np.random.default_rng(0).integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - 120.0
    plan = model.stage_inputs([img, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))])
    return model, plan


def step_and_stages(backbone, dtype, B, H, Wd, steps):
    """ the whole step, and the stem + backbone ops alone (the leading ops of the plan, as the plan runs them: side lanes included) """
    model, plan = staged(backbone, dtype, B, H, Wd)
    step = time_us(lambda: model.run_plan(plan), steps)
    n_bb = sum(1 for kind, _, _, name, _ in plan.ops if R.Plan.stage_of(kind, name) in (1, 2))
    assert all(R.Plan.stage_of(k, n) in (1, 2) for k, _, _, n, _ in plan.ops[:n_bb])
    st = hip.stream_ptr

    def backbone_only():
        hip.check(hip.lib().gpp_plan_run(plan.array, n_bb, st(), None, 0), 'gpp_plan_run')
    bb = time_us(backbone_only, steps)
    rec = {'what': 'step', 'backbone': backbone, 'dtype': dtype, 'batch': B, 'hw': [H, Wd], 'images_per_s': round(B * 1e6 / step, 1),
           'ms_per_step': round(step / 1e3, 3), 'stem_backbone_ms': round(bb / 1e3, 3), 'stem_backbone_launches': n_bb,
           'anchors_per_image': plan.n_anchors}
    return model, plan, rec


def block_rows(model, plan, dtype, steps):
    """ every fused block of the plan: time, compulsory bytes, TB/s, GFLOP/s """
    rows = []
    for index, (kind, _, desc, name, flops) in enumerate(plan.ops):
        if kind not in (R.OP_MOBILENET_BLOCK, R.OP_MOBILENET_STEM):
            continue
        us = time_us(lambda: model.run_op(plan, index), steps)
        if kind == R.OP_MOBILENET_STEM:
            ho, wo = M.out_size(desc.H, 2), M.out_size(desc.W, 2)
            nbytes = 4.0 * desc.B * (desc.H * desc.W * 3 + ho * wo * desc.C_out)
            shape = '3x3/2 3 -> {} at {}x{}x{}'.format(desc.C_out, desc.B, desc.H, desc.W)
            tile = 0
        else:
            nbytes = M.block_bytes(desc)
            shape = 'dw/{} {} -> {} at {}x{}x{}'.format(desc.stride, desc.C_in, desc.C_out, desc.B, desc.H, desc.W)
            tile = int(desc.tile_hint)
        rows.append({'what': 'block', 'layer': name, 'dtype': dtype, 'shape': shape, 'tile': tile, 'us': round(us, 1),
                     'compulsory_MB': round(nbytes / 1e6, 1), 'TB_per_s': round(nbytes / us / 1e6, 2), 'TFLOP_per_s': round(flops / us / 1e6, 1)})
    return rows


def fused_vs_two_launches(model, plan, dtype, steps, how_many=3):
    """ the blocks with the largest maps: the fused launch against depthwise-to-HBM + a plain 1x1 conv (gpp_conv2d_igemm with a ReLU
    epilogue, its best tile: the same bytes and FLOPs as a ReLU6 one) on the same input """
    blocks = [(i, op) for i, op in enumerate(plan.ops) if op[0] == R.OP_MOBILENET_BLOCK]
    blocks.sort(key=lambda t: -M.block_bytes(t[1][2]))
    dev = torch.device('cuda')
    rows = []
    for index, (kind, _, d, name, _) in blocks[:how_many]:
        fused = time_us(lambda: model.run_op(plan, index), steps)
        ho, wo = M.out_size(d.H, d.stride), M.out_size(d.W, d.stride)
        mid = torch.empty((d.B, ho, wo, d.C_in), dtype=torch.float32, device=dev)
        out = torch.empty((d.B, ho, wo, d.C_out), dtype=torch.float32, device=dev)
        k = (np.random.default_rng(0).standard_normal((1, 1, d.C_in, d.C_out)) / np.sqrt(d.C_in)).astype(np.float32)
        wt, bias = C.pack_weight(k, dtype, dev), torch.zeros(d.C_out, device=dev)
        osc = C.out_scale_of(k, dev) if dtype == 'f16x3' else None
        cd = C.conv_desc([C.FMap(mid, d.B, ho, wo, d.C_in)], [C.FMap(out, d.B, ho, wo, d.C_out)], wt, bias, 1, 1, d.C_in, d.C_out, relu=True,
                         dtype=dtype, out_scale=osc)
        best = ctypes.c_float(0.0)
        lib = hip.lib()

        def depthwise():
            hip.check(lib.gpp_mobilenet_depthwise(ctypes.c_void_p(d.inp), ctypes.c_void_p(d.dw_weight), ctypes.c_void_p(d.dw_bias),
                                                  ctypes.c_void_p(mid.data_ptr()), d.B, d.H, d.W, d.C_in, d.stride, d.in_pitch, d.C_in,
                                                  hip.stream_ptr()), 'gpp_mobilenet_depthwise')
        depthwise()
        hip.check(lib.gpp_conv2d_autotune(ctypes.byref(cd), 8, hip.stream_ptr(), ctypes.byref(best)), 'autotune')

        def two():
            depthwise()
            hip.check(lib.gpp_conv2d_igemm(ctypes.byref(cd), hip.stream_ptr()), 'gpp_conv2d_igemm')
        dw_us = time_us(depthwise, steps)
        two_us = time_us(two, steps)
        rows.append({'what': 'fused_vs_two', 'layer': name, 'dtype': dtype, 'fused_us': round(fused, 1), 'two_launch_us': round(two_us, 1),
                     'depthwise_us': round(dw_us, 1), 'pointwise_us': round(two_us - dw_us, 1), 'fused_over_two': round(fused / two_us, 3),
                     'fused_tile': int(d.tile_hint), 'pointwise_tile': int(cd.tile_hint)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--backbone', default='mobilenet224_1.0')
    ap.add_argument('--against', default='resnet50')
    ap.add_argument('--dtypes', default='f16x3,f32')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--hw', default='402,1333')
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    H, Wd = (int(v) for v in a.hw.split(','))
    sink = open(a.out, 'a') if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()
    for dtype in a.dtypes.split(','):
        model, plan, rec = step_and_stages(a.backbone, dtype, a.batch, H, Wd, a.steps)
        emit(rec)
        for row in block_rows(model, plan, dtype, a.steps) + fused_vs_two_launches(model, plan, dtype, a.steps):
            emit(row)
        del model, plan
        torch.cuda.empty_cache()
        _, _, other = step_and_stages(a.against, dtype, a.batch, H, Wd, a.steps)
        emit(other)
        emit({'what': 'verdict', 'dtype': dtype, 'mobilenet_faster_than_{}'.format(a.against): rec['ms_per_step'] < other['ms_per_step'],
              'step_ratio': round(rec['ms_per_step'] / other['ms_per_step'], 3)})
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
