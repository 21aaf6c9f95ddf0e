"""
Layer 0 of the regression tower on the 9 x 9 candidate set: what gpp_detect_deep_lists lists at radius 4 on the frames
bench.py runs, and what the two launches that replace the fused pyramid_towers_0 cost against it.

For the flagship plan (ResNet-50, f16x3, B x 402 x 1333) this reports the rows of the radius-2, -3 and -4 lists as shares of the pyramid with their
flags, and times with HIP events: the 384-column launch of a depth-4 plan, its regression slice gathered on the frames' lists and dense (flag forced
to 1), the list launches alone, and the fused 896-column launch of a depth-3 plan of the same model.

    python tools/bench_tower0.py [--batch 8] [--iters 30] > profiles/tower0/counts_and_launches.txt
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
    import torch
    from keras_retinanet_3D import models
    from keras_retinanet_3D.backend import hip
    from keras_retinanet_3D.models import retinanet as R
    from keras_retinanet_3D.utils import synthetic

    B = args.batch
    planes = synthetic.load_plane_database('1k').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    inputs = [synthetic.synthetic_network_input(list(range(B))), np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
    lib = hip.lib()

    def load(depth):
        os.environ['GPP_SPARSE_TOWER_DEPTH'] = str(depth)
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype=args.dtype)
        model.predict_on_batch(inputs)
        torch.cuda.synchronize()
        return model, model.plan_for(B, inputs[0].shape[1], inputs[0].shape[2], planes.shape[0], True)

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

    def op_runner(plan, name):
        index = [op[3] for op in plan.ops].index(name)
        op = ctypes.byref(plan.array, index * ctypes.sizeof(R.PlanOp))
        return lambda: hip.check(lib.gpp_plan_run(op, 1, hip.stream_ptr(), None, 0))

    model4, four = load(4)
    sp = four.sparse
    if sp is None or sp.tower0 is None:
        raise SystemExit('this plan does not take the form (see head_forms in models/plan.py)')
    G = hip.GPP_MAX_GROUPS
    total = B * sum(sp.level_pixels)
    stats = sp.deep_stats.cpu().numpy().tolist()
    n2, n3, n4 = int(sp.deep_counts[0][G].item()), int(sp.deep_counts[1][G].item()), int(sp.tower0_counts[G].item())
    print('# {} {} B = {}: {} pyramid rows, limit {} rows'.format(model4.backbone_name, args.dtype, B, total, sp.deep_max_rows))
    print('# marks {} ({:.2%}), radius 1 {} ({:.2%}), radius 2 {} ({:.2%}), radius 3 {} ({:.2%}), radius 4 = the rows of layer 0 {} ({:.2%})'.format(
        stats[0], stats[0] / total, stats[1], stats[1] / total, n2, n2 / total, n3, n3 / total, n4, n4 / total))
    print('# flags: layer 2 {}, layer 1 {}, layer 0 {};  radius 4 per level: {}'.format(
        int(sp.deep_flags[0].item()), int(sp.deep_flags[1].item()), int(sp.tower0_flag.item()),
        sp.tower0_counts.cpu().numpy()[:len(sp.level_pixels)].tolist()))
    print('\nHIP events, us')
    print('  the 384-column launch of pyramid_towers_0 (tile {}): {:.1f}'.format(
        four.tuning.get('pyramid_towers_0@cols', (0, 0))[0], time_call(op_runner(four, 'pyramid_towers_0'))))
    handle = sp.tower0_handle
    run_slice = lambda: hip.check(lib.gpp_conv2d_deferred_run(handle, 0, hip.stream_ptr()))      # noqa: E731
    sp.tower0_flag.fill_(0)
    rows_us = time_call(run_slice)
    sp.tower0_flag.fill_(1)
    dense_us = time_call(run_slice)
    print('  the regression slice: gathered on {} rows (with its idle dense twin) {:.1f}, dense (with its idle gathered twin) {:.1f}, ratio {:.2f}'.format(
        n4, rows_us, dense_us, rows_us / dense_us))
    lists = four.ops[[op[3] for op in four.ops].index('pyramid_classification')][2].lists_after
    print('  the four list launches alone: {:.1f}'.format(time_call(lambda: hip.check(lib.gpp_detect_deep_lists_run(lists, 0, hip.stream_ptr())))))
    sp.reset(torch)
    model3, three = load(3)
    print('  the fused 896-column launch of a depth-3 plan (tile {}): {:.1f}'.format(
        three.tuning.get('pyramid_towers_0', (0, 0))[0], time_call(op_runner(three, 'pyramid_towers_0'))))
    print('  the four list launches of a depth-3 plan alone: {:.1f}'.format(time_call(lambda: hip.check(lib.gpp_detect_deep_lists_run(
        three.ops[[op[3] for op in three.ops].index('pyramid_classification')][2].lists_after, 0, hip.stream_ptr())))))
    three.sparse.reset(torch)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
