#!/usr/bin/env python3
"""
Measures the tracker's ego-motion compensation (gpp_track_ego_f64) beside the entry points without it on one GPU,
in ONE process:

  1. the launch alone, alternating at each point: gpp_track_f64 / gpp_track_optimal_f64 against gpp_track_ego_f64 with the same
     assignment and IDENTITY records -- the same matches and the same work behind step 1, so the difference is step 1b itself, the 13
     words per frame and the records' copy.  One sequence of N = 8 frames, HIP events around each launch, median of 200.  The points are
     tools/bench_track_optimal.py's without its dense one: D = 100 entered with 0, 50 and 128 occupied slots for dist and bev, and a
     KITTI-like frame of 15 cars;
  2. at B = 8, resnet50, the 1k plane database, 375 x 1242: ms per predict_tracks_on_frames call of a model with and a model without
     'ego', alternating;
  3. no GPU: the driving scenes of tests/track_ego_oracle.py tracked with and without their records and scored against their own ground
     truth (utils/mot_eval.evaluate_sequences, BEV overlap, hota=True, idf1=True).

--launches-only stops after 1 and takes the plain entry points alone when the library (GPP_LIB) has no gpp_track_ego_f64: that is how
two builds are compared, alternating processes in one session (profiles/track_ego/README.md).  --scenes-only runs 3 alone.

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_track_ego.jsonl (one JSON record per measurement) and <out>/tables.md; <out> defaults to profiles/track_ego.

    python tools/bench_track_ego.py [--out DIR] [--steps 30] [--warmup 5] [--rounds 3] [--dtype f16x3] [--launches-only] [--scenes-only]
                                    [--no-model] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from keras_retinanet_3D.utils import mot_eval  # noqa: E402
from keras_retinanet_3D.utils import track as T  # noqa: E402

ASSIGNS = ('greedy', 'optimal')
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] + [0.0] * 7


def launches_alone(records, tag):
    import torch
    import bench_track as B
    import bench_track_optimal as BO
    from keras_retinanet_3D.backend import hip
    dev = hip.require_device()
    has_ego = hasattr(hip.lib(), 'gpp_track_ego_f64')
    for name, option, host, entry, reps in BO.points()[:-1]:
        N, D = host.shape[:2]
        work = torch.empty((hip.track_ego_workspace_bytes(1, N) if has_ego else hip.track_workspace_bytes(1),), dtype=torch.uint8, device=dev)
        ego = np.array([IDENTITY] * N)
        rows = torch.as_tensor(host).to(dev)
        out, ids, hits = torch.empty_like(rows), torch.empty((N, D), dtype=torch.int32, device=dev), torch.empty((N, D), dtype=torch.int32, device=dev)
        params = T.params_of(option)
        state, nxt = T.state_tensor(entry, dev), T.state_tensor(None, dev)
        for assign in ASSIGNS:
            want = T.track_rows_np(host, dict(T.check_option(option), assign=assign), entry)
            for entry_point in ('plain', 'ego') if has_ego else ('plain',):
                with B.step_limit(120, '{}, {}, {}, {}'.format(name, option[0], assign, entry_point)):
                    more = {'ego': ego} if entry_point == 'ego' else {}
                    med, low = B.median_us(lambda: hip.track(rows, state, params, state_out=nxt, out=out, ids=ids, hits=hits, workspace=work,
                                                             optimal=assign == 'optimal', **more), n=reps, warm=reps // 10)
                    same = ids.cpu().numpy().tolist() == want[1].tolist() and bool((T.read_state(nxt)[0]['box'] == want[3]['box']).all())
                    records.append({'what': 'track launch', 'tag': tag, 'point': name, 'assign': assign, 'entry_point': entry_point,
                                    'metric': option[0], 'threshold': option[1], 'N': N, 'D': D,
                                    'occupied_at_entry': int((entry['id1'] != 0).sum()), 'matched_rows': int((want[2] > 1).sum()),
                                    'median_us': round(med, 2), 'min_us': round(low, 2), 'us_per_frame': round(med / N, 2),
                                    'equals_host_form': bool(same)})


def model_step(records, args):
    import torch
    import bench_track as B
    from keras_retinanet_3D import models
    from keras_retinanet_3D.models import weights as W
    from keras_retinanet_3D.utils import synthetic
    Bn, h, w = 8, 375, 1242
    option = {'metric': 'dist', 'threshold': 2.0}
    ego = np.array([IDENTITY] * Bn)
    with B.step_limit(900, 'building the models and their plans'):
        weights = W.synthetic_weights('resnet50', 1234)
        run = {'plain': models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=option),
               'ego': models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=dict(option, ego=True))}
        more = {'plain': {}, 'ego': {'ego': ego}}
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        frames = (np.random.default_rng(0).integers(0, 2, size=(Bn, h, w, 3)) * 255).astype(np.uint8)
        call = [frames, np.tile(P_inv[None].astype(np.float32), (Bn, 1, 1)), np.tile(planes[None], (Bn, 1, 1))]
        for _ in range(args.warmup):
            for a in run:
                (rows, counts, _, _), _ = run[a].predict_tracks_on_frames(*call, **more[a])
    for r in range(args.rounds):
        for a in run:
            with B.step_limit(300, 'predict_tracks_on_frames, {}, round {}'.format(a, r)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run[a].predict_tracks_on_frames(*call, **more[a])
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1000.0 / args.steps
                records.append({'what': 'model call', 'model': a, 'round': r, 'B': Bn, 'frame': [h, w], 'dtype': args.dtype,
                                'ms_per_call': round(ms, 3), 'images_per_s': round(Bn * 1000.0 / ms, 1), 'rows': int(counts.sum())})


def scored(records):
    import bench_track_optimal as BO
    import track_ego_oracle as E
    import track_oracle as O
    for scene, build in (('curve: 1.5 m and 0.04 rad per frame', E.curve), ('the curve with 0.01 rad of pitch per frame', E.pitching),
                         ('straight: 2.5 m per frame', E.straight), ('the curve, two of the cars moving 0.4 m per frame', E.with_movers)):
        frames, ego, gts = build()
        labels = BO.labels_of(frames, gts)
        for metric, thr in E.FOR:
            for assign in ASSIGNS:
                for records_given in (False, True):
                    option = dict(O.options(metric, thr), **({'assign': 'optimal'} if assign == 'optimal' else {}))
                    rows, ids, _, state = T.track_rows_np(frames, option, ego=ego if records_given else None)
                    res = mot_eval.evaluate_sequences([labels], [(rows, ids)], metric='bev', hota=True, idf1=True)['all']
                    records.append({'what': 'scene scored', 'scene': scene, 'metric': metric, 'threshold': thr, 'assign': assign,
                                    'records': records_given, 'cars': E.CARS, 'ids_given': int(state['next_id']),
                                    'switches_by_row': T.id_switches(gts, ids), 'IDS': res['ids'], 'MOTA': round(res['mota'], 4),
                                    'IDF1': round(res['idf1']['idf1'], 4), 'AssA': round(float(res['hota']['assa']), 4),
                                    'HOTA': round(float(res['hota']['hota']), 4),
                                    'max_velocity_component': round(float(np.abs(state['box'][7:10]).max()), 4)})


def tables(records):
    out = ['| point | metric | assignment | entry point | N | D | slots at entry | matched rows | median us | min us | us per frame | == host form |',
           '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'track launch':
            out.append('| {point} | {metric} | {assign} | {entry_point} | {N} | {D} | {occupied_at_entry} | {matched_rows} | {median_us} | {min_us} | '
                       '{us_per_frame} | {equals_host_form} |'.format(**r))
    out += ['', '| predict_tracks_on_frames, B = 8 | round | ms per call | images/s | rows |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'model call':
            out.append('| {model} | {round} | {ms_per_call} | {images_per_s} | {rows} |'.format(**r))
    out += ['', '| scene | option | assignment | records | ids given (8 cars) | IDS | MOTA | IDF1 | AssA | HOTA | largest velocity component |',
            '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'scene scored':
            out.append('| {scene} | {metric} {threshold} | {assign} | {records} | {ids_given} | {IDS} | {MOTA} | {IDF1} | {AssA} | {HOTA} | '
                       '{max_velocity_component} |'.format(**r))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_ego'))
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    ap.add_argument('--launches-only', action='store_true')
    ap.add_argument('--scenes-only', action='store_true')
    ap.add_argument('--no-model', action='store_true')
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    os.environ.setdefault('GPP_AUTOTUNE', '0')
    os.makedirs(args.out, exist_ok=True)
    records = []
    if not args.scenes_only:
        launches_alone(records, args.tag)
        if not args.launches_only and not args.no_model:
            model_step(records, args)
    if not args.launches_only:
        scored(records)
    name = 'launches_{}.jsonl'.format(args.tag) if args.launches_only else 'scenes.jsonl' if args.scenes_only else 'bench_track_ego.jsonl'
    with open(os.path.join(args.out, name), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    if not args.launches_only and not args.scenes_only:
        with open(os.path.join(args.out, 'tables.md'), 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
