"""
Mixed KITTI frame sizes as one batch against the ways the same frames ran before, in one process: ResNet-50 at B = 8 with
two frames of each KITTI size (375x1242, 370x1224, 374x1238, 376x1241 -> network inputs of 402, 403, 403 and 404 x 1333), per dtype

  (a) the ragged batch: one call of the ragged plan of the class (101, 1333);
  (b) the same eight frames grouped by network-input shape: three calls (2 x 402, 4 x 403, 2 x 404 rows), their plans built and warm -- what
      the frames cost without the ragged form once no plan is built inside the call any more.  (b4: grouped by RAW shape, as bin/run_network.py
      grouped them: four calls of two, two of them on the same plan);
  (c) a uniform batch of eight 404 x 1333 inputs.

    python tools/bench_ragged.py [--dtypes f16x3,f32] [--steps 20] [--out FILE]
Timing: device events around `steps` back-to-back plan runs on inputs resident in HBM, after a warm-up of every plan; five windows per leg, the
legs alternated inside every window; a leg's figure is the median of its windows, its spread their max - min.  The verdicts use the spread of (b)
as the margin: (a) <= (b) + spread, |(a) - (c)| <= spread.  Also recorded, per dtype: how many plans each way builds and the seconds of building
them (buffers + tile tuning, the one-off cost inside a first call), and the stem's own time in (a) and (c).  One JSON line per record.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.models import retinanet as R  # noqa: E402
from keras_retinanet_3D.utils import image as I  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402

RAW = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
BGR_MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def window_us(fns, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        for fn in fns:
            fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def measure(legs, iters, windows=5):
    """ legs: {name: [callables of one step]} -> {name: (median us, spread us, [windows])}, the legs alternated inside every window """
    for fns in legs.values():
        for _ in range(2):
            for fn in fns:
                fn()
    torch.cuda.synchronize()
    got = {name: [] for name in legs}
    for _ in range(windows):
        for name, fns in legs.items():
            got[name].append(window_us(fns, iters))
    return {name: (float(np.median(v)), float(max(v) - min(v)), [round(x, 1) for x in v]) for name, v in got.items()}


def bench(dtype, steps, emit):
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype=dtype)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv1 = synthetic.synthetic_calibration()
    raw = [s for s in RAW for _ in range(2)]                                    # two frames of each size
    heights = [I.resized_shape(s)[0] for s in raw]
    assert len(I.split_by_height_class(raw)) == 1 and sorted(set(heights)) == [402, 403, 404]
    rng = np.random.default_rng(0)
    base = [rng.integers(0, 256, size=(404, 1333, 3)).astype(np.float32) - BGR_MEAN for _ in raw]
    frames = [b[:h] for b, h in zip(base, heights)]

    def calib(n):
        return np.tile(P_inv1[None].astype(np.float32), (n, 1, 1)), np.tile(planes[None], (n, 1, 1))

    def build(inputs):
        t0 = time.time()
        plan = model.stage_inputs(inputs)
        torch.cuda.synchronize()
        return plan, time.time() - t0

    # the one-off cost: the plans each way builds for these eight frames (buffers + tile tuning), timed as the first call pays them
    ragged, ragged_s = build([frames] + list(calib(8)))
    by_shape, build_s = {}, 0.0
    for h in sorted(set(heights)):
        group = [f for f, fh in zip(frames, heights) if fh == h]
        by_shape[h], s = build([np.stack(group)] + list(calib(len(group))))
        build_s += s
    by_raw = []
    for s in RAW:
        group = [f for f, r in zip(frames, raw) if r == s]
        plan, sec = build([np.stack(group)] + list(calib(len(group))))       # (a second plan object for the same key is the same plan: no new build)
        by_raw.append(plan)
    n_before = len(model._plans)
    raw_plans = len(set(id(p) for p in by_raw))
    uniform, _ = build([np.stack(base)] + list(calib(8)))
    emit({'what': 'one_off', 'dtype': dtype, 'ragged_plans': 1, 'ragged_build_s': round(ragged_s, 2), 'by_shape_plans': len(by_shape),
          'by_shape_build_s': round(build_s, 2), 'by_raw_shape_calls': len(by_raw), 'by_raw_shape_plans': raw_plans,
          'plans_in_model': n_before, 'autotune': os.environ.get('GPP_AUTOTUNE', '1') != '0'})

    # every leg runs on inputs resident in its plans' buffers (the two 403-row groups of b4 share one plan, and its last staged frames)
    run = model.run_plan
    legs = {'a_ragged': [lambda: run(ragged)],
            'b_by_shape': [(lambda p: (lambda: run(p)))(p) for p in by_shape.values()],
            'b4_by_raw_shape': [(lambda p: (lambda: run(p)))(p) for p in by_raw],
            'c_uniform_404': [lambda: run(uniform)]}
    res = measure(legs, steps)
    a, b, c = res['a_ragged'], res['b_by_shape'], res['c_uniform_404']
    margin = b[1]
    for name, (med, spread, wins) in res.items():
        emit({'what': 'leg', 'dtype': dtype, 'leg': name, 'batch': 8, 'us_per_step': round(med, 1), 'spread_us': round(spread, 1), 'windows_us': wins,
              'images_per_s': round(8e6 / med, 1), 'calls': len(legs[name])})
    # the stem alone (the leading ops of stage 1), ragged against uniform at the class's largest height
    def stem_of(plan):
        n = sum(1 for kind, _, _, name, _ in plan.ops if R.Plan.stage_of(kind, name) == 1)
        return [lambda: [model.run_op(plan, i) for i in range(n)]]
    stem = measure({'ragged': stem_of(ragged), 'uniform_404': stem_of(uniform)}, steps)
    emit({'what': 'stem', 'dtype': dtype, 'ragged_us': round(stem['ragged'][0], 1), 'uniform_404_us': round(stem['uniform_404'][0], 1),
          'ragged_spread_us': round(stem['ragged'][1], 1), 'uniform_spread_us': round(stem['uniform_404'][1], 1)})
    emit({'what': 'verdict', 'dtype': dtype, 'a_over_b': round(a[0] / b[0], 4), 'a_over_c': round(a[0] / c[0], 4), 'margin_us': round(margin, 1),
          'a_not_slower_than_b': bool(a[0] <= b[0] + margin), 'a_equals_c_within_margin': bool(abs(a[0] - c[0]) <= margin)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtypes', default='f16x3,f32')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sink = open(a.out, 'a') if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()
    for dtype in a.dtypes.split(','):
        bench(dtype, a.steps, emit)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
