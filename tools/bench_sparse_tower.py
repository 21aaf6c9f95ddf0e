"""
Sparse regression tower: where the gathered launch of pyramid_regression_3 crosses its dense launch, and how much
of the pyramid the layers in front of it would have to compute.

For the flagship plan (ResNet-50, f16x3, B x 402 x 1333) this reports, on the frames bench.py runs, the share of pyramid rows that carry a
candidate, the share inside its 3 x 3 dilation (the device's own dilated lists, checked against NumPy) and inside the 5 x 5 one (what a
gathered pyramid_regression_2 would have to write), and times with HIP events, launch by launch,
  * the layer's dense launch (the lists' flag set) and what the idle twin of either form costs,
  * its gathered launch at 1/8, 1/4, 0.4, 1/2, 0.6 and 3/4 of the rows (random ascending lists) and on the bench frames' own dilated lists, for the
    height the device chooses (8000256) and for every fixed height,
  * the list launches behind the candidate pass with and without the dilation.

    python tools/bench_sparse_tower.py [--batch 8] [--iters 30] > profiles/sparse_tower/crossover.txt
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

TILES = (8000256, 8128256, 8160256, 8192256, 8224256, 8256256)


def dilate(mask):
    padded = np.zeros((mask.shape[0], mask.shape[1] + 2, mask.shape[2] + 2), bool)
    padded[:, 1:-1, 1:-1] = mask
    out = np.zeros_like(mask)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= padded[:, dy:dy + mask.shape[1], dx:dx + mask.shape[2]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--dtype', default='f16x3')
    args = ap.parse_args()
    os.environ['GPP_SPARSE_HEADS'] = '1'
    os.environ['GPP_SPARSE_TOWER'] = '1'
    os.environ['GPP_SPARSE_TOWER_DEPTH'] = '1'        # the layers in front stay dense here (tools/bench_deep_tower.py measures them gathered)
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
    if sp is None or sp.tower_rows is None:
        raise SystemExit('this plan does not run its regression tower sparse (batch too small for the one-round rule?)')
    torch.cuda.synchronize()
    counts, rows = sp.counts.cpu().numpy(), sp.rows.cpu().numpy()
    t_counts, t_rows = sp.tower_counts.cpu().numpy(), sp.tower_rows.cpu().numpy().copy()
    total = B * sum(sp.level_pixels)
    print('# {} {} B = {}: {} pyramid rows; {} carry a candidate ({:.2%}); the device\'s dilated lists hold {} ({:.2%}); guards at {} / {} rows; '
          'flags = {} / {}'.format(model.backbone_name, args.dtype, B, total, int(counts[-1]), counts[-1] / total, int(t_counts[-1]), t_counts[-1] / total,
                                   sp.max_rows, sp.tower_max_rows, int(sp.flag.item()), int(sp.tower_flag.item())))
    shapes = [(plan.features['P{}'.format(i + 3)].H, plan.features['P{}'.format(i + 3)].W) for i in range(5)]
    begin, once, twice = 0, 0, 0
    for l, (h, w) in enumerate(shapes):
        mask = np.zeros((B * h * w,), bool)
        mask[rows[begin:begin + counts[l]]] = True
        d1 = dilate(mask.reshape(B, h, w))
        d2 = dilate(d1)
        same = np.array_equal(np.flatnonzero(d1.reshape(-1)), t_rows[begin:begin + t_counts[l]])
        print('#   level {} ({} x {}): {} listed, {} in the 3 x 3 dilation (device list {}), {} in the 5 x 5 one'.format(
            l, h, w, int(counts[l]), int(d1.sum()), 'equal' if same else 'DIFFERS', int(d2.sum())))
        once, twice, begin = once + int(d1.sum()), twice + int(d2.sum()), begin + B * h * w
    print('# 3 x 3 dilation: {} rows ({:.2%}); 5 x 5 dilation (what a gathered pyramid_regression_2 would write): {} rows ({:.2%})'.format(
        once, once / total, twice, twice / total))

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

    index = [i for i, (kind, _, desc, _, _) in enumerate(plan.ops) if kind == R.OP_CONV and desc.tower_rows][0]
    desc = plan.ops[index][2]
    plain = [i for i, op in enumerate(plan.ops) if op[3] == 'pyramid_regression_2'][0]
    print('\n{} (dense tile {}, gathered tile {}); pyramid_regression_2 beside it: {:.1f} us'.format(
        plan.ops[index][3], desc.tile_hint, desc.tower_tile, time_op(plain)))
    sp.tower_flag.fill_(1)
    dense_us = time_op(index)
    sp.tower_counts.zero_()
    sp.tower_flag.fill_(0)
    idle_us = time_op(index)
    sp.tower_flag.fill_(2)
    off_us = time_op(index)
    print('  dense launch + idle gathered twin {:8.1f} us    nothing listed (idle dense twin + empty gathered launch) {:.1f} us    both switched off {:.1f} us'.format(
        dense_us, idle_us, off_us))
    sp.tower_flag.fill_(0)
    rng = np.random.default_rng(0)

    def put(lists):
        buf, begin = np.zeros((total,), np.int32), 0
        for p, lst in zip(sp.level_pixels, lists):
            buf[begin:begin + len(lst)] = lst
            begin += B * p
        sp.tower_rows.copy_(torch.as_tensor(buf))
        n = [len(x) for x in lists]
        sp.tower_counts.copy_(torch.as_tensor(n + [0] * (hip.GPP_MAX_GROUPS - len(n)) + [sum(n)], dtype=torch.int32))
        return sum(n)

    cases = [('{:.3f} of the rows, random'.format(s), [np.sort(rng.choice(B * p, size=int(B * p * s), replace=False)) for p in sp.level_pixels])
             for s in (0.125, 0.25, 0.4, 0.5, 0.6, 0.75)]
    own, begin = [], 0
    for l, p in enumerate(sp.level_pixels):
        own.append(t_rows[begin:begin + t_counts[l]])
        begin += B * p
    cases.append(('the bench frames\' dilated lists', own))
    print('  {:>34} {:>8} '.format('lists', 'rows') + ' '.join('{:>9}'.format(t) for t in TILES) + '   best vs dense')
    for name, lists in cases:
        n = put(lists)
        us = []
        for tile in TILES:
            desc.tower_tile = tile
            us.append(time_op(index))
        print('  {:>34} {:>8} '.format(name, n) + ' '.join('{:>9.1f}'.format(u) for u in us) + '   {:.2f}x (device\'s choice {:.2f}x)'.format(
            min(us) / dense_us, us[0] / dense_us))
    desc.tower_tile = plan.tuning.get(plan.ops[index][3] + '@rows', (0, 0.0))[0]
    # the list launches with and without the dilation
    model.predict_on_batch(inputs)
    torch.cuda.synchronize()
    cand = [i for i, op in enumerate(plan.ops) if op[0] == R.OP_DETECT_CANDIDATE_PIXELS][0]
    d = plan.ops[cand][2]

    def time_lists(lists):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.check(lib.gpp_detect_pixel_lists(ctypes.byref(lists), hip.stream_ptr()))
        e0.record()
        for _ in range(args.iters):
            lib.gpp_detect_pixel_lists(ctypes.byref(lists), hip.stream_ptr())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / args.iters
    both = time_lists(d.lists)
    alone = type(d.lists).from_buffer_copy(d.lists)
    alone.dilated_bitmap = alone.dilated_rows = alone.dilated_counts = alone.dilated_flag = None
    print('\ncandidate pass + lists {:.1f} us per step; the list launches alone {:.1f} us, without the dilated lists {:.1f} us (on the candidates\' lane, '
          'under pyramid_regression_1 / 2)'.format(time_op(cand), both, time_lists(alone)))
    sp.reset(torch)


if __name__ == '__main__':
    main()
