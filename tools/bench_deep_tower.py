"""
Deep sparse regression tower: what gpp_detect_deep_lists lists on the frames bench.py runs, and what layers 1 and 2 of
the regression tower cost on those lists.

For the flagship plan (ResNet-50, f16x3, B x 402 x 1333) this reports the marks, their 3 x 3 dilation and the rows of the radius-2 and radius-3
lists as shares of the pyramid (the marks against the candidate pass's own lists, the radius-1 count against its dilated lists), the flags, and
times with HIP events, op by op as the plan runs them: pyramid_regression_1 / 2 / 3 gathered on the frames' lists and dense (flag forced to
1), pyramid_classification with and without the list launches behind it, and the list launches alone.

    python tools/bench_deep_tower.py [--batch 8] [--iters 30] > profiles/deep_tower/counts_and_launches.txt
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
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--dtype', default='f16x3')
    args = ap.parse_args()
    os.environ['GPP_SPARSE_TOWER_DEPTH'] = '3'
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
    if sp is None or sp.deep_layers < 2:
        raise SystemExit('this plan does not take the deep form (see head_forms in models/plan.py)')
    torch.cuda.synchronize()
    G = hip.GPP_MAX_GROUPS
    total = B * sum(sp.level_pixels)
    stats = sp.deep_stats.cpu().numpy().tolist()
    n2, n3 = int(sp.deep_counts[0][G].item()), int(sp.deep_counts[1][G].item())
    print('# {} {} B = {}: {} pyramid rows'.format(model.backbone_name, args.dtype, B, total))
    print('# marks {} ({:.2%}; the candidate pass lists {}), 3 x 3 dilation {} ({:.2%}; its dilated lists hold {}), f3 = {}'.format(
        stats[0], stats[0] / total, int(sp.counts[G].item()), stats[1], stats[1] / total, int(sp.tower_counts[G].item()), stats[2]))
    print('# radius 2 (the rows of pyramid_regression_2): {} ({:.2%}), flag {};  radius 3 (pyramid_regression_1): {} ({:.2%}), flag {};  limit {} rows'.format(
        n2, n2 / total, int(sp.deep_flags[0].item()), n3, n3 / total, int(sp.deep_flags[1].item()), sp.deep_max_rows))
    for k, name in ((0, 'radius 2'), (1, 'radius 3')):
        print('#   {} per level: {}'.format(name, sp.deep_counts[k].cpu().numpy()[:len(sp.level_pixels)].tolist()))
    lib = hip.lib()
    names = [op[3] for op in plan.ops]

    def time_call(fn, iters=args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e30
        for _ in range(3):
            fn()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1000.0 / iters)
        return best

    def op_runner(index):
        op = ctypes.byref(plan.array, index * ctypes.sizeof(R.PlanOp))
        return lambda: hip.check(lib.gpp_plan_run(op, 1, hip.stream_ptr(), None, 0))

    print('\nop by op, HIP events, us (gathered: on the lists above, with the idle dense twin; dense: flag 1, with the idle gathered twin)')
    flags = {'pyramid_regression_1': sp.deep_flags[1], 'pyramid_regression_2': sp.deep_flags[0], 'pyramid_regression_3': sp.tower_flag}
    for name, flag in flags.items():
        run = op_runner(names.index(name))
        flag.fill_(0)
        rows_us = time_call(run)
        flag.fill_(1)
        dense_us = time_call(run)
        flag.fill_(0)
        print('  {:22s} gathered {:7.1f}   dense {:7.1f}   ratio {:.2f}'.format(name, rows_us, dense_us, rows_us / dense_us))
    cls = names.index('pyramid_classification')
    desc = plan.ops[cls][2]
    with_lists = time_call(op_runner(cls))
    handle, desc.lists_after = desc.lists_after, 0
    without = time_call(op_runner(cls))
    desc.lists_after = handle
    lists = time_call(lambda: hip.check(lib.gpp_detect_deep_lists_run(handle, 0, hip.stream_ptr())))
    print('  pyramid_classification with the list launches behind it {:.1f}, without {:.1f}; the four list launches alone {:.1f}'.format(with_lists, without, lists))
    sp.reset(torch)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
