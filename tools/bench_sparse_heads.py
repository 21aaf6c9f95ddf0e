"""
Sparse head outputs: where the gathered launch of a head output layer crosses its dense launch.

For the two output layers of the flagship plan (ResNet-50, f16x3, B x 402 x 1333) this times, launch by launch with HIP events,
  * the dense launch (its guard set),
  * the gathered launch on lists holding every n-th pixel of every level, n = 64 .. 1 (row share 1/n),
  * both launches switched off by the guard (what the idle twin of a pair costs a step),
  * the two list launches behind the candidate pass,
and reports, on the frames bench.py runs, the share of pyramid pixels that carry a candidate and the share inside the 3 x 3 dilation
of that set (what a gathered form of the layer BEFORE the output layer would have to compute).

    python tools/bench_sparse_heads.py [--batch 8] [--iters 50] > profiles/sparse_heads/crossover.txt
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--dtype', default='f16x3')
    args = ap.parse_args()
    os.environ['GPP_SPARSE_HEADS'] = '1'
    import torch
    from keras_retinanet_3D import models
    from keras_retinanet_3D.backend import hip
    from keras_retinanet_3D.models import retinanet as R
    from keras_retinanet_3D.utils import synthetic

    B = args.batch
    planes = synthetic.load_plane_database('1k').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    inputs = [synthetic.synthetic_network_input(list(range(B))), np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype=args.dtype)
    model.predict_on_batch(inputs)
    plan = model.plan_for(B, inputs[0].shape[1], inputs[0].shape[2], planes.shape[0], True)
    sp = plan.sparse
    torch.cuda.synchronize()
    counts = sp.counts.cpu().numpy()
    rows = sp.rows.cpu().numpy()
    total = B * sum(sp.level_pixels)
    print('# {} {} B = {}: {} pyramid pixels, {} carry a candidate ({:.2%}); guard at {} rows ({:.2%}); flag = {}'.format(
        model.backbone_name, args.dtype, B, total, int(counts[-1]), counts[-1] / total, sp.max_rows, sp.max_rows / total, int(sp.flag.item())))
    # the 3 x 3 dilation of the candidate set, level by level
    shapes = [(plan.features['P{}'.format(i + 3)].H, plan.features['P{}'.format(i + 3)].W) for i in range(5)]
    begin, dilated = 0, 0
    for l, (h, w) in enumerate(shapes):
        mask = np.zeros((B, h + 2, w + 2), bool)
        lst = rows[begin:begin + counts[l]]
        b, p = np.divmod(lst, h * w)
        y, x = np.divmod(p, w)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                mask[b, y + dy, x + dx] = True
        n = int(mask[:, 1:-1, 1:-1].sum())
        print('#   level {} ({} x {}): {} listed, {} in the 3 x 3 dilation'.format(l, h, w, int(counts[l]), n))
        dilated += n
        begin += B * h * w
    print('# 3 x 3 dilation of the candidate set: {} pixels ({:.2%} of all; the listed set itself {:.2%})'.format(dilated, dilated / total, counts[-1] / total))

    lib = hip.lib()

    def time_op(index, iters=args.iters):
        op = ctypes.byref(plan.array, index * ctypes.sizeof(R.PlanOp))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e30
        for _ in range(3):
            hip.check(lib.gpp_plan_run(op, 1, hip.stream_ptr(), None, 0))
            e0.record()
            for _ in range(iters):
                lib.gpp_plan_run(op, 1, hip.stream_ptr(), None, 0)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1000.0 / iters)
        return best

    pairs = [(i - 1, i) for i, (kind, _, desc, _, _) in enumerate(plan.ops) if kind == R.OP_CONV and desc.gather_rows]
    for dense_i, rows_i in pairs:
        name = plan.ops[rows_i][3]
        print('\n{} (dense tile {}, gathered tile {})'.format(name, plan.ops[dense_i][2].tile_hint, plan.ops[rows_i][2].tile_hint))
        sp.flag.fill_(1)
        dense_us = time_op(dense_i)
        off_rows = time_op(rows_i)
        sp.flag.fill_(0)
        off_dense = time_op(dense_i)
        print('  dense launch {:8.1f} us    switched off: dense {:.1f} us, gathered {:.1f} us'.format(dense_us, off_dense, off_rows))
        print('  {:>8} {:>9} {:>12} {:>10}'.format('1/n', 'rows', 'gathered us', 'vs dense'))
        for n in (64, 32, 16, 12, 8, 6, 4, 3, 2, 1):
            sp.put_every_nth(torch, n)
            us = time_op(rows_i)
            print('  {:>8} {:>9} {:>12.1f} {:>9.2f}x'.format('1/{}'.format(n), int(sp.counts[-1].item()), us, us / dense_us))
    # the candidate pass with and without the two list launches behind it
    model.predict_on_batch(inputs)
    torch.cuda.synchronize()
    cand = [i for i, op in enumerate(plan.ops) if op[0] == R.OP_DETECT_CANDIDATE_PIXELS][0]
    with_lists = time_op(cand)
    d = plan.ops[cand][2]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hip.check(lib.gpp_detect_pixel_lists(ctypes.byref(d.lists), hip.stream_ptr()))
    e0.record()
    for _ in range(args.iters):
        lib.gpp_detect_pixel_lists(ctypes.byref(d.lists), hip.stream_ptr())
    e1.record()
    e1.synchronize()
    print('\ncandidate pass + pixel lists {:.1f} us per step, of which the two list launches {:.1f} us (on the candidates\' lane, under the regression tower)'.format(
        with_lists, e0.elapsed_time(e1) * 1000.0 / args.iters))
    sp.reset(torch)


if __name__ == '__main__':
    main()
