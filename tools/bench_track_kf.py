#!/usr/bin/env python3
"""
Measures the tracker's Kalman filter (gpp_track_kf_f64) beside the entry points without it on one GPU, in ONE
process:

  1. the launch alone, alternating at each point: gpp_track_f64 / gpp_track_optimal_f64 (`plain`), gpp_track_ego_f64 with IDENTITY
     records (`ego`) and gpp_track_kf_f64 with the same records, once under the point's own metric with the filter (`kf`) and once under
     'maha' at 3 standard deviations (`kf maha`).  One sequence of N = 8 frames, HIP events around each launch, median of 200.  The
     points are tools/bench_track_optimal.py's: a KITTI-like frame of 15 cars and D = 100 entered with 0, 50 and 128 occupied slots, for
     dist and bev, greedy and optimal.  The ratio kf / ego is recorded, not asserted;
  2. at B = 8, resnet50, the 1k plane database, 375 x 1242: ms per predict_tracks_on_frames call of a model with and a model without the
     filter, alternating;
  3. no GPU: a seeded synthetic set -- cars at 8 - 70 m seen from one driving camera, their positions disturbed along and across the
     viewing ray by the noise model's own sigmas, misses -- tracked with every 'dist' threshold of a sweep and with 'maha', both with
     the camera's ego records, and scored against its own ground truth (utils/mot_eval.evaluate_sequences, BEV overlap, hota=True,
     idf1=True).  The best 'dist' threshold is the one of the highest HOTA.  Synthetic data only: no real checkpoint or KITTI sequence.

--launches-only stops after 1 and takes the entry points the library (GPP_LIB) has: that is how two builds are compared, alternating
processes in one session (profiles/track_kf/README.md).  --scenes-only runs 3 alone.

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_track_kf.jsonl (one JSON record per measurement) and <out>/tables.md; <out> defaults to profiles/track_kf.

    python tools/bench_track_kf.py [--out DIR] [--steps 30] [--warmup 5] [--rounds 3] [--dtype f16x3] [--launches-only] [--scenes-only]
                                   [--no-model] [--tag NAME]
"""
import argparse
import json
import math
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
# the values of the issue's demonstration; nothing here has seen a real sequence
NOISE = {'radial': (0.1, 0.05), 'tangential': (0.1, 0.005), 'process': (0.01, 0.01), 'birth_speed': 2.0}
GATE = 3.0
SWEEP = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0)


def with_filter(option, maha=False):
    metric, thr = ('maha', GATE) if maha else option
    return {'metric': metric, 'threshold': thr, 'filter': 'kalman', 'noise': NOISE}


def launches_alone(records, tag):
    import torch
    import bench_track as B
    import bench_track_optimal as BO
    from keras_retinanet_3D.backend import hip
    dev = hip.require_device()
    has_ego, has_kf = hasattr(hip.lib(), 'gpp_track_ego_f64'), hasattr(hip.lib(), 'gpp_track_kf_f64')
    entry_points = ['plain'] + (['ego'] if has_ego else []) + (['kf', 'kf maha'] if has_kf else [])
    for name, option, host, entry, reps in BO.points()[:-1]:
        N, D = host.shape[:2]
        work = torch.empty((hip.track_ego_workspace_bytes(1, N) if has_ego else hip.track_workspace_bytes(1),), dtype=torch.uint8, device=dev)
        ego = np.array([IDENTITY] * N)
        rows = torch.as_tensor(host).to(dev)
        out, ids, hits = torch.empty_like(rows), torch.empty((N, D), dtype=torch.int32, device=dev), torch.empty((N, D), dtype=torch.int32, device=dev)
        occupied = int((entry['id1'] != 0).sum())
        first = None if occupied == 0 else B.grid(128, occupied, 1)[None] if D == 100 else B.grid(16, 15, 1)[None]
        for assign in ASSIGNS:
            for entry_point in entry_points:
                kalman = entry_point.startswith('kf')
                opt = with_filter(option, entry_point == 'kf maha') if kalman else {'metric': option[0], 'threshold': option[1]}
                opt = dict(T.check_option(opt), **({'assign': 'optimal'} if assign == 'optimal' else {}))
                begin = (T.empty_state(), T.empty_cov()) if first is None else (T.track_rows_np(first, opt) + (None,))[3:5]
                want = T.track_rows_np(host, opt, begin[0], ego=ego if entry_point != 'plain' else None, **({'cov': begin[1]} if kalman else {}))
                state, nxt = T.state_tensor(begin[0], dev), T.state_tensor(None, dev)
                more = {} if entry_point == 'plain' else {'ego': ego}
                if kalman:
                    more.update(kf=T.kf_params_of(opt), cov_in=T.cov_tensor(begin[1], dev), cov_out=T.cov_tensor(None, dev))
                params = T.params_of(opt)
                with B.step_limit(120, '{}, {}, {}, {}'.format(name, option[0], assign, entry_point)):
                    med, low = B.median_us(lambda: hip.track(rows, state, params, state_out=nxt, out=out, ids=ids, hits=hits, workspace=work,
                                                             optimal=assign == 'optimal', **more), n=reps, warm=reps // 10)
                    same = ids.cpu().numpy().tolist() == want[1].tolist() and bool((T.read_state(nxt)[0]['box'] == want[3]['box']).all())
                    if kalman:
                        same = same and bool((T.read_cov(more['cov_out'])[0] == want[4]).all())
                    records.append({'what': 'track launch', 'tag': tag, 'point': name, 'assign': assign, 'entry_point': entry_point,
                                    'point_metric': option[0], 'metric': opt['metric'], 'threshold': opt['threshold'], 'N': N, 'D': D, 'occupied_at_entry': occupied,
                                    'matched_rows': int((want[2] > 1).sum()), 'median_us': round(med, 2), 'min_us': round(low, 2),
                                    'us_per_frame': round(med / N, 2), 'equals_host_form': bool(same)})


def model_step(records, args):
    import torch
    import bench_track as B
    from keras_retinanet_3D import models
    from keras_retinanet_3D.models import weights as W
    from keras_retinanet_3D.utils import synthetic
    Bn, h, w = 8, 375, 1242
    option = {'metric': 'dist', 'threshold': 2.0}
    with B.step_limit(900, 'building the models and their plans'):
        weights = W.synthetic_weights('resnet50', 1234)
        run = {'fixed': models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=option),
               'kalman': models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=with_filter(('dist', 2.0))),
               'kalman maha': models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=with_filter(None, True))}
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        frames = (np.random.default_rng(0).integers(0, 2, size=(Bn, h, w, 3)) * 255).astype(np.uint8)
        call = [frames, np.tile(P_inv[None].astype(np.float32), (Bn, 1, 1)), np.tile(planes[None], (Bn, 1, 1))]
        for _ in range(args.warmup):
            for a in run:
                (rows, counts, _, _), _ = run[a].predict_tracks_on_frames(*call)
    for r in range(args.rounds):
        for a in run:
            with B.step_limit(300, 'predict_tracks_on_frames, {}, round {}'.format(a, r)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run[a].predict_tracks_on_frames(*call)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1000.0 / args.steps
                records.append({'what': 'model call', 'model': a, 'round': r, 'B': Bn, 'frame': [h, w], 'dtype': args.dtype,
                                'ms_per_call': round(ms, 3), 'images_per_s': round(Bn * 1000.0 / ms, 1), 'rows': int(counts.sum())})


def synthetic_set(seed=0, frames=60, cars=24, D=32, miss=0.15, speed=1.0, yaw=0.01):
    """ `cars` cars on four lanes (x = -7.5, -3.5, 3.5, 7.5 m in the world) between 10 and 130 m ahead, a third of them moving +-0.3 m per
    frame along the road, seen from a camera that drives `speed` metres and turns `yaw` rad per frame.  A car is in the frame while its
    range is 8 - 70 m and it lies ahead; its position is disturbed along its viewing ray by sigma_r = radial0 + radial1 rho and across
    it by sigma_t = tangential0 + tangential1 rho (NOISE: the filter is given the true noise model), and it is missed with probability
    `miss`.  -> (frames (N, D, 36), ego (N, 16), per frame the car of every row) """
    import track_ego_oracle as E
    from track_oracle import padding, row
    rng = np.random.default_rng(seed)
    lanes = (-7.5, -3.5, 3.5, 7.5)
    world = [np.array([lanes[k % 4] + rng.uniform(-0.3, 0.3), 1.65, rng.uniform(10.0, 130.0), 1.0]) for k in range(cars)]
    vel = [np.array([0.0, 0.0, (0.3 if k % 2 else -0.3) if k % 3 == 0 else 0.0, 0.0]) for k in range(cars)]
    dims, ry = rng.uniform([3.4, 1.5, 1.4], [4.8, 1.9, 1.8], (cars, 3)), rng.uniform(-0.1, 0.1, cars)
    advance = E.rot_y(yaw)
    advance[2, 3] = speed
    pose, before = np.eye(4), np.eye(4)
    out, ego, gts = [], [], []
    (r0, r1), (t0, t1) = NOISE['radial'], NOISE['tangential']
    for f in range(frames):
        rel = np.linalg.inv(pose).dot(before)
        dyaw = math.atan2(rel[0, 2] - rel[2, 0], rel[0, 0] + rel[2, 2])
        ego.append(E.record(rel[:3, :3], rel[:3, 3], dyaw))
        ry = ry + dyaw
        to_camera = np.linalg.inv(pose)
        seen = []
        for k in range(cars):
            p = to_camera.dot(world[k] + f * vel[k])[:3]
            rho = math.hypot(p[0], p[2])
            if not (8.0 <= rho <= 70.0 and p[2] > 0.0) or rng.uniform() < miss:
                continue
            u = np.array([p[0] / rho, p[2] / rho])
            along, across = rng.normal(0.0, r0 + r1 * rho), rng.normal(0.0, t0 + t1 * rho)
            x, z = p[0] + along * u[0] - across * u[1], p[2] + along * u[1] + across * u[0]
            seen.append((k, row(0.9, x, z, dims[k][0], dims[k][1], ry[k], dims[k][2], p[1], 0)))
        frame, gt, order = padding(D), np.full(D, -1, np.int64), rng.permutation(D)
        for j, (k, r) in enumerate(seen[:D]):
            frame[order[j]], gt[order[j]] = r, k
        out.append(frame)
        gts.append(gt)
        before, pose = pose, pose.dot(advance)
    return np.stack(out), np.array(ego), gts


def scored(records):
    import bench_track_optimal as BO
    for seed in (0, 1, 2):
        frames, ego, gts = synthetic_set(seed)
        labels = BO.labels_of(frames, gts)
        cars = len({int(k) for g in gts for k in g if k >= 0})
        options = [('dist', thr, {'metric': 'dist', 'threshold': thr}) for thr in SWEEP] + [('maha', GATE, with_filter(None, True))]
        for assign in ASSIGNS:
            for metric, thr, option in options:
                option = dict(option, **({'assign': 'optimal'} if assign == 'optimal' else {}))
                res = T.track_rows_np(frames, option, ego=ego)
                rows, ids, state = res[0], res[1], res[3]
                score = mot_eval.evaluate_sequences([labels], [(rows, ids)], metric='bev', hota=True, idf1=True)['all']
                records.append({'what': 'synthetic set scored', 'seed': seed, 'metric': metric, 'threshold': thr, 'assign': assign,
                                'frames': len(frames), 'cars_seen': cars, 'rows': int(sum((g >= 0).sum() for g in gts)),
                                'ids_given': int(state['next_id']), 'switches_by_row': T.id_switches(gts, ids), 'IDS': score['ids'],
                                'MOTA': round(score['mota'], 4), 'IDF1': round(score['idf1']['idf1'], 4),
                                'AssA': round(float(score['hota']['assa']), 4), 'HOTA': round(float(score['hota']['hota']), 4)})


def tables(records):
    out = ['| point | metric | assignment | entry point | N | D | slots at entry | matched rows | median us | min us | us per frame | == host form |',
           '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'track launch':
            out.append('| {point} | {metric} | {assign} | {entry_point} | {N} | {D} | {occupied_at_entry} | {matched_rows} | {median_us} | {min_us} | '
                       '{us_per_frame} | {equals_host_form} |'.format(**r))
    out += ['', '| point | metric | assignment | ego, us per frame | kf, us per frame | kf / ego | kf maha / ego |', '|---|---|---|---|---|---|---|']
    launch = {(r['point'], r['point_metric'], r['assign'], r['entry_point']): r['us_per_frame'] for r in records if r['what'] == 'track launch'}
    for (point, metric, assign, entry_point), ego in launch.items():
        if entry_point == 'ego' and (point, metric, assign, 'kf') in launch:
            kf, maha = launch[(point, metric, assign, 'kf')], launch[(point, metric, assign, 'kf maha')]
            out.append('| {} | {} | {} | {} | {} | {:.3f} | {:.3f} |'.format(point, metric, assign, ego, kf, kf / ego, maha / ego))
    out += ['', '| predict_tracks_on_frames, B = 8 | round | ms per call | images/s | rows |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'model call':
            out.append('| {model} | {round} | {ms_per_call} | {images_per_s} | {rows} |'.format(**r))
    out += ['', '| seed | option | assignment | frames | cars seen | rows | ids given | IDS | MOTA | IDF1 | AssA | HOTA |',
            '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'synthetic set scored':
            out.append('| {seed} | {metric} {threshold} | {assign} | {frames} | {cars_seen} | {rows} | {ids_given} | {IDS} | {MOTA} | {IDF1} | {AssA} | '
                       '{HOTA} |'.format(**r))
    out += ['', '| seed | assignment | best dist threshold (by HOTA) | its ids, IDS, MOTA, IDF1, AssA, HOTA | maha 3.0: ids, IDS, MOTA, IDF1, AssA, HOTA |',
            '|---|---|---|---|---|']
    line = lambda r: '{ids_given}, {IDS}, {MOTA}, {IDF1}, {AssA}, {HOTA}'.format(**r)  # noqa: E731
    sets = [r for r in records if r['what'] == 'synthetic set scored']
    for seed in sorted({r['seed'] for r in sets}):
        for assign in ASSIGNS:
            mine = [r for r in sets if r['seed'] == seed and r['assign'] == assign]
            best = max((r for r in mine if r['metric'] == 'dist'), key=lambda r: r['HOTA'])
            maha = [r for r in mine if r['metric'] == 'maha'][0]
            out.append('| {} | {} | {} | {} | {} |'.format(seed, assign, best['threshold'], line(best), line(maha)))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_kf'))
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
    name = 'launches_{}.jsonl'.format(args.tag) if args.launches_only else 'scenes.jsonl' if args.scenes_only else 'bench_track_kf.jsonl'
    with open(os.path.join(args.out, name), 'a' if args.launches_only else 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    if not args.launches_only and not args.scenes_only:
        with open(os.path.join(args.out, 'tables.md'), 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
