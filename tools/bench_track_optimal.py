#!/usr/bin/env python3
"""
Measures the tracker's optimal assignment (gpp_track_optimal_f64) beside the greedy one (gpp_track_f64) on one
GPU, in ONE process:

  1. the launch alone, either entry point at each point, alternating: one sequence of N = 8 frames, HIP events around each launch,
     median of 200 (50 at the dense point).  The points: D = 100 on tools/bench_track.py's grid entered with 0, 50 and 128 occupied
     slots, for dist and bev; a KITTI-like frame of 15 cars; and the most the rule allows -- 128 slots x 128 rows, every pair a candidate
     at equal cells (dist, identical rows).  The launch always goes from the same entry state to a second buffer;
  2. at B = 8, resnet50, the 1k plane database, 375 x 1242: ms per predict_tracks_on_frames call with either assignment, alternating,
     and track_rows_np with either assignment on the rows of such a call;
  3. no GPU: the dense drive of tests/track_optimal_oracle.py scored against its own ground truth (utils/mot_eval.evaluate_sequences,
     BEV overlap, hota=True, idf1=True) with either assignment.

--launches-only stops after 1 and takes the greedy entry point alone when the library (GPP_LIB) has no gpp_track_optimal_f64: that is
how two builds are compared, alternating processes in one session (profiles/track_optimal/README.md).

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_track_optimal.jsonl (one JSON record per measurement) and <out>/tables.md; <out> defaults to profiles/track_optimal.

    python tools/bench_track_optimal.py [--out DIR] [--steps 30] [--warmup 5] [--rounds 3] [--dtype f16x3] [--launches-only] [--tag NAME]
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
import torch  # noqa: E402

import bench_track as B  # noqa: E402
from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.models import weights as W  # noqa: E402
from keras_retinanet_3D.utils import mot_eval  # noqa: E402
from keras_retinanet_3D.utils import synthetic  # noqa: E402
from keras_retinanet_3D.utils import track as T  # noqa: E402

ASSIGNS = ('greedy', 'optimal')


def points():
    """ [(name, option, frames (N, D, 36), entry state, repetitions)] """
    out = []
    for metric in ('dist', 'bev'):
        option = (metric, B.THRESHOLDS[metric])
        host = np.stack([B.grid(100, 100, 10 + f) for f in range(8)])
        for occupied in (0, 50, 128):
            entry = T.track_rows_np(B.grid(128, occupied, 1)[None], option)[3] if occupied else T.empty_state()
            out.append(('grid D = 100, {} slots at entry'.format(occupied), option, host, entry, 200))
    option = ('dist', 2.0)
    host = np.stack([B.grid(16, 15, 40 + f) for f in range(8)])
    out.append(('15 cars, D = 16', option, host, T.track_rows_np(B.grid(16, 15, 1)[None], option)[3], 200))
    same = np.tile(B.grid(1, 1, 0), (128, 1))
    host = np.stack([same] * 8)
    out.append(('128 x 128, every pair a candidate at equal cells', option, host, T.track_rows_np(same[None], option)[3], 50))
    return out


def launches_alone(records, tag):
    dev = hip.require_device()
    work = torch.empty((hip.track_workspace_bytes(1),), dtype=torch.uint8, device=dev)
    assigns = [a for a in ASSIGNS if a == 'greedy' or hasattr(hip.lib(), 'gpp_track_optimal_f64')]
    for name, option, host, entry, reps in points():
        N, D = host.shape[:2]
        rows = torch.as_tensor(host).to(dev)
        out, ids, hits = torch.empty_like(rows), torch.empty((N, D), dtype=torch.int32, device=dev), torch.empty((N, D), dtype=torch.int32, device=dev)
        params = T.params_of(option)
        state, nxt = T.state_tensor(entry, dev), T.state_tensor(None, dev)
        for assign in assigns:
            with B.step_limit(120, '{}, {}, {}'.format(name, option[0], assign)):
                best = assign == 'optimal'
                med, low = B.median_us(lambda: hip.track(rows, state, params, state_out=nxt, out=out, ids=ids, hits=hits, workspace=work,
                                                         optimal=best), n=reps, warm=reps // 10)
                want = T.track_rows_np(host, dict(T.check_option(option), assign=assign), entry)
                same = ids.cpu().numpy().tolist() == want[1].tolist() and T.read_state(nxt)[0].tobytes() == want[3].tobytes()
                records.append({'what': 'track launch', 'tag': tag, 'point': name, 'assign': assign, 'metric': option[0], 'threshold': option[1],
                                'N': N, 'D': D, 'occupied_at_entry': int((entry['id1'] != 0).sum()), 'matched_rows': int((want[2] > 1).sum()),
                                'median_us': round(med, 2), 'min_us': round(low, 2), 'us_per_frame': round(med / N, 2),
                                'equals_host_form': bool(same)})


def model_step(records, args):
    Bn, h, w = 8, 375, 1242
    option = {'metric': 'dist', 'threshold': 2.0}
    with B.step_limit(900, 'building the models and their plans'):
        weights = W.synthetic_weights('resnet50', 1234)
        run = {a: models.load_model(weights, backbone_name='resnet50', dtype=args.dtype, pose=True, track=dict(option, assign=a)) for a in ASSIGNS}
        planes = synthetic.load_plane_database('1k').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        frames = (np.random.default_rng(0).integers(0, 2, size=(Bn, h, w, 3)) * 255).astype(np.uint8)
        call = [frames, np.tile(P_inv[None].astype(np.float32), (Bn, 1, 1)), np.tile(planes[None], (Bn, 1, 1))]
        for _ in range(args.warmup):
            for a in ASSIGNS:
                (rows, counts, _, _), _ = run[a].predict_tracks_on_frames(*call)
    for r in range(args.rounds):
        for a in ASSIGNS:
            with B.step_limit(300, 'predict_tracks_on_frames, {}, round {}'.format(a, r)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    run[a].predict_tracks_on_frames(*call)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1000.0 / args.steps
                records.append({'what': 'model call', 'assign': a, 'round': r, 'B': Bn, 'frame': [h, w], 'dtype': args.dtype,
                                'ms_per_call': round(ms, 3), 'images_per_s': round(Bn * 1000.0 / ms, 1), 'rows': int(counts.sum())})
    (pose, _), _ = run['greedy'].predict_poses_on_frames(*call)
    state = run['greedy'].track_state()
    for a in ASSIGNS:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            T.track_rows_np(pose, dict(option, assign=a), state)
        ms = (time.perf_counter() - t0) * 1000.0 / args.steps
        records.append({'what': 'track_rows_np', 'assign': a, 'B': Bn, 'rows': int(counts.sum()), 'occupied_at_entry': int((state['id1'] != 0).sum()),
                        'ms_per_call': round(ms, 3), 'ms_per_frame': round(ms / Bn, 3)})


def labels_of(frames, gts):
    """ the drive's own rows as KITTI labels: (labels per frame (A, 16), track ids per frame) """
    per_frame, ids = [], []
    for rows, g in zip(frames, gts):
        k = np.flatnonzero(g >= 0)
        r, lab = rows[k].astype(np.float64), np.zeros((k.size, mot_eval.LABEL_COLS))
        lab[:, 3], lab[:, 4:8] = r[:, 25], r[:, 26:30]
        lab[:, 8], lab[:, 9], lab[:, 10], lab[:, 11], lab[:, 12], lab[:, 13], lab[:, 14] = (r[:, c] for c in (30, 17, 18, 19, 31, 21, 32))
        per_frame.append(lab)
        ids.append(g[k])
    return per_frame, ids


def scored(records):
    import track_optimal_oracle as P
    import track_oracle as O
    frames, gts = P.dense_drive(with_gt=True)
    labels = labels_of(frames, gts)
    for a in ASSIGNS:
        rows, ids, _, state = T.track_rows_np(frames, dict(O.options('dist'), assign=a))
        res = mot_eval.evaluate_sequences([labels], [(rows, ids)], metric='bev', hota=True, idf1=True)['all']
        records.append({'what': 'dense drive scored', 'assign': a, 'ids_given': int(state['next_id']), 'switches_by_row': T.id_switches(gts, ids),
                        'IDS': res['ids'], 'MOTA': round(res['mota'], 4), 'IDF1': round(res['idf1']['idf1'], 4),
                        'AssA': round(float(res['hota']['assa']), 4), 'HOTA': round(float(res['hota']['hota']), 4), 'tp': res['tp'], 'fn': res['fn'],
                        'fp': res['fp']})


def tables(records):
    out = ['| point | metric | assignment | N | D | slots at entry | matched rows | median us | min us | us per frame | == host form |',
           '|---|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'track launch':
            out.append('| {point} | {metric} | {assign} | {N} | {D} | {occupied_at_entry} | {matched_rows} | {median_us} | {min_us} | {us_per_frame} | '
                       '{equals_host_form} |'.format(**r))
    out += ['', '| predict_tracks_on_frames, B = 8 | round | ms per call | images/s | rows |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'model call':
            out.append('| {assign} | {round} | {ms_per_call} | {images_per_s} | {rows} |'.format(**r))
    out += ['', '| track_rows_np on the rows of one such call | rows | slots at entry | ms per call | ms per frame |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'track_rows_np':
            out.append('| {assign} | {rows} | {occupied_at_entry} | {ms_per_call} | {ms_per_frame} |'.format(**r))
    out += ['', '| dense drive, scored | ids given | IDS | MOTA | IDF1 | AssA | HOTA | tp | fn | fp |', '|---|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'dense drive scored':
            out.append('| {assign} | {ids_given} | {IDS} | {MOTA} | {IDF1} | {AssA} | {HOTA} | {tp} | {fn} | {fp} |'.format(**r))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_optimal'))
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dtype', default='f16x3')
    ap.add_argument('--launches-only', action='store_true')
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    os.environ.setdefault('GPP_AUTOTUNE', '0')
    hip.require_device()
    os.makedirs(args.out, exist_ok=True)
    records = []
    launches_alone(records, args.tag)
    if not args.launches_only:
        model_step(records, args)
        scored(records)
    name = 'launches_{}.jsonl'.format(args.tag) if args.launches_only else 'bench_track_optimal.jsonl'
    with open(os.path.join(args.out, name), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    if not args.launches_only:
        with open(os.path.join(args.out, 'tables.md'), 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
