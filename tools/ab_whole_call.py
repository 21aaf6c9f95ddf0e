#!/usr/bin/env python3
"""
One leg of an A/B of the scores' host side between two checkouts of this repository, each with its library built: the "whole call" step
of tools/bench_hota.py and tools/bench_idf1.py (default sizes: 8000 frames; the stress set of 32 frames for HOTA) and the call with both
scores, on the tree TREE -- median of 7 wall-clock calls after a warm one, every call ends in a download.  Prints one JSON line; the
caller alternates the two trees, one fresh process per leg (profiles/pair_tables/README.md).

    python tools/ab_whole_call.py TREE LABEL REPEAT
"""
import json
import os
import statistics
import sys
import time

tree, label, repeat = os.path.abspath(sys.argv[1]), sys.argv[2], int(sys.argv[3])
for p in (os.path.join(tree, 'ground-plane-polling_amd'), tree, os.path.join(tree, 'tools')):
    sys.path.insert(0, p)

from bench_mot_eval import kitti_sized, stress  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import mot_eval as M  # noqa: E402

assert os.path.abspath(M.__file__).startswith(tree) and os.path.abspath(hip.LIB_PATH).startswith(tree), (M.__file__, hip.LIB_PATH)
hip.require_device()


def timed(labels, tracks, **score):
    M.evaluate_sequences(labels, tracks, device=True, **score)                  # (warm: the library, the allocator)
    t_with, t_without = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        M.evaluate_sequences(labels, tracks, device=True, **score)
        t_with.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        M.evaluate_sequences(labels, tracks, device=True)
        t_without.append(time.perf_counter() - t0)
    return {'with_ms': round(statistics.median(t_with) * 1e3, 2), 'without_ms': round(statistics.median(t_without) * 1e3, 2),
            'with_min_ms': round(min(t_with) * 1e3, 2), 'with_max_ms': round(max(t_with) * 1e3, 2)}


kitti = kitti_sized(8000)
record = {'tree': label, 'repeat': repeat, 'lib': hip.lib().gpp_version().decode(),
          'hota_kitti': timed(*kitti, hota=True), 'hota_stress': timed(*stress(32), hota=True),
          'idf1_kitti': timed(*kitti, idf1=True), 'both_kitti': timed(*kitti, hota=True, idf1=True)}
print(json.dumps(record))
