#!/usr/bin/env python3
"""
Measures several road planes per frame (utils/road_fit.py fit_rounds_*, csrc/road_fit.hip gpp_road_peel_i32) on one GPU, in
ONE process, on the `--frames` (64) synthetic scans of tools/bench_road_fit.py ('flat') and on the same scans with the far half turned
into a ramp ('ramp': beyond z = 25 m the road rises 1 in 16; fitted with height = (1.0, 4.0), because the ramp's plane extended back to the
camera has d = h + 25 / 16, about 3.2 m).  H = `--hypotheses` (1 024), P = 1, 2, 3.

  (a) HIP events around gpp_road_peel_i32 (its three launches, with the allocation and clearing of the result tensors, as the other
      launches' times in profiles/road_fit) after round 0 and after round 1
  (b) HIP events around a round's score / winner / moments launches, rounds 0, 1, 2 (each on that round's points)
  (c) fit_rounds_device per frame against fit_rounds_np on the same frames, P = 1, 2, 3, and fit_device (what P = 1 must cost);
      device == host is checked for every P
  (d) on the ramp set, per round: the planes found against the two true planes of the frame (each plane is compared with the nearer
      truth: height error at the segment's centre, x = 0 and z = 12.5 m or 37.5 m, and the angle between the normals), and the inlier
      share (inliers / kept_0) of every round, the first spurious one included -- recorded, not asserted; min_share = 0 for this leg, so
      that the spurious rounds are seen

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_road_fit_rounds.jsonl and the tables of <out>/README.md between its two markers; <out> defaults to profiles/road_fit_rounds.
None of these figures is asserted anywhere: they are records.

    python tools/bench_road_fit_rounds.py [--out DIR] [--frames 64] [--points 120000] [--hypotheses 1024]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_kitti_eval import launch_times, step_limit  # noqa: E402
from bench_road_fit import VELO_TO_CAM, synthetic_scan  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import road_fit  # noqa: E402

BEGIN, END = '<!-- bench_road_fit_rounds: begin -->', '<!-- bench_road_fit_rounds: end -->'
BREAK_Z, RISE = 25.0, 1.0 / 16.0


def ramp_scan(scan, truth):
    """ the scan with the road beyond z = BREAK_Z rising 1 in 16 (y points down: it decreases), and the ramp's true plane """
    R, t = VELO_TO_CAM[:, :3], VELO_TO_CAM[:, 3]
    cam = scan[:, :3].astype(np.float64) @ R.T + t
    cam[:, 1] -= np.maximum(0.0, cam[:, 2] - BREAK_Z) * RISE
    out = scan.copy()
    out[:, :3] = ((cam - t) @ np.linalg.inv(R).T).astype(np.float32)
    a, c, h = -truth[0] / truth[1], -truth[2] / truth[1], -truth[3] / truth[1]
    ramp = np.array([a, -1.0, c - RISE, h + BREAK_Z * RISE])
    return out, ramp / np.linalg.norm(ramp[:3])


def against(plane, truth, z):
    height = lambda p: -(p[2] * z + p[3]) / p[1]  # noqa: E731
    return abs(height(plane) - height(truth)), float(np.arccos(np.clip(plane[:3] @ truth[:3], -1.0, 1.0)))


def readme_tables(records):
    pick = lambda what, **kw: [r for r in records if r['what'] == what and all(r[k] == v for k, v in kw.items())]  # noqa: E731
    s = pick('setup')[0]
    lines = ['`tools/bench_road_fit_rounds.py`, one MI355X, one process; library `{}`.'.format(s['library']), '',
             '{} synthetic frames of {} points, H = {}; `flat`: the scans of `tools/bench_road_fit.py` ({:.0f} kept per frame); `ramp`: the same with '
             'the road rising 1 in 16 beyond z = 25 m, fitted with `height=(1.0, 4.0)` ({:.0f} kept per frame).'.format(
                 s['frames'], s['points'], s['hypotheses'], s['kept_mean']['flat'], s['kept_mean']['ramp']), '',
             '| launch alone (HIP events, the {} frames as one chunk), median us (min) | flat | ramp |'.format(s['frames']), '|---|---|---|']
    names = []
    for r in pick('launch_alone', set='flat'):
        names.append((r['launch'], r['round']))
    for name, rnd in names:
        cells = ['{} ({})'.format(r['median_us'], r['min_us']) for r in [pick('launch_alone', set=k, launch=name, round=rnd)[0] for k in ('flat', 'ramp')]]
        lines.append('| `{}`, round {} | {} | {} |'.format(name, rnd, *cells))
    lines += ['', '| whole fit, ms per frame | flat | ramp | device == host |', '|---|---|---|---|']
    for r in pick('wall', set='flat'):
        o = pick('wall', set='ramp', form=r['form'], P=r['P'])[0]
        lines.append('| `{}`{} | {:.2f} | {:.2f} | {} |'.format(r['form'], '' if r['P'] is None else ', P = {}'.format(r['P']), r['ms_per_frame'], o['ms_per_frame'],
                                                          '' if r['equal'] is None else ('yes' if r['equal'] and o['equal'] else 'NO')))
    lines += ['', 'The ramp set, P = 3 and `min_share = 0`, per round over the {} frames -- recorded, not asserted.  Each plane is compared with the '
              'nearer of the frame\'s two true planes: the height error at the segment\'s centre (x = 0; z = 12.5 m on the flat part, 37.5 m on the ramp) and '
              'the angle between the normals.'.format(s['frames']), '',
              '| round | frames with a plane | on the flat part / on the ramp | height error median (max) mm | angle median (max) rad | inlier share median (min .. max) |',
              '|---|---|---|---|---|---|']
    for r in pick('ramp_round'):
        lines.append('| {} | {} | {} / {} | {:.2f} ({:.2f}) | {:.2e} ({:.2e}) | {:.3f} ({:.3f} .. {:.3f}) |'.format(
            r['round'], r['planes'], r['on_flat'], r['on_ramp'], r['height_median_m'] * 1e3, r['height_max_m'] * 1e3, r['angle_median_rad'], r['angle_max_rad'],
            r['share_median'], r['share_min'], r['share_max']))
    f = pick('flat_round')
    lines += ['', 'The flat set, P = 3 and `min_share = 0`: inlier share per round, median (min .. max): ' +
              '; '.join('round {}: {:.3f} ({:.3f} .. {:.3f})'.format(r['round'], r['share_median'], r['share_min'], r['share_max']) for r in f) + '.']
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'road_fit_rounds'))
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--hypotheses', type=int, default=1024)
    args = ap.parse_args()
    dev = hip.require_device()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records = []

    def note(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    rng = np.random.default_rng(2022)
    made = [synthetic_scan(rng, args.points) for _ in range(args.frames)]
    flat, flat_truth = [m[0] for m in made], np.stack([m[1] for m in made])
    ramped = [ramp_scan(s, t) for s, t in made]
    sets = {'flat': (flat, dict(hypotheses=args.hypotheses)),
            'ramp': ([m[0] for m in ramped], dict(hypotheses=args.hypotheses, height=(1.0, 4.0)))}
    ramp_truth = np.stack([m[1] for m in ramped])
    F = args.frames
    Ts, ids = [VELO_TO_CAM] * F, list(range(F))
    kept_mean, free = {}, {}

    for name, (scans, options) in sets.items():
        o = road_fit.resolve_options(**options)
        # ---- (c) the whole fit; the first call also warms every launch up
        with step_limit(240, 'fit_device ' + name):
            road_fit.fit_rounds_device(scans[:2], Ts[:2], ids[:2], 3, **options)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one = road_fit.fit_device(scans, Ts, ids, **options)
            note({'what': 'wall', 'set': name, 'form': 'fit_device', 'P': None, 'ms_per_frame': round((time.perf_counter() - t0) / F * 1e3, 3), 'equal': None})
        kept_mean[name] = float(np.mean(one['kept']))
        for P in (1, 2, 3):
            with step_limit(240, 'fit_rounds_device ' + name):
                t0 = time.perf_counter()
                got = road_fit.fit_rounds_device(scans, Ts, ids, P, **options)
                dev_s = time.perf_counter() - t0
            with step_limit(600, 'fit_rounds_np ' + name):
                t0 = time.perf_counter()
                want = road_fit.fit_rounds_np(scans, Ts, ids, P, **options)
                np_s = time.perf_counter() - t0
            equal = all(got[k].tobytes() == want[k].tobytes() for k in want)
            if P == 1:
                equal = equal and all(np.ascontiguousarray(got[k][:, 0]).tobytes() == one[k].tobytes() for k in one)
            note({'what': 'wall', 'set': name, 'form': 'fit_rounds_device', 'P': P, 'ms_per_frame': round(dev_s / F * 1e3, 3), 'equal': bool(equal)})
            note({'what': 'wall', 'set': name, 'form': 'fit_rounds_np', 'P': P, 'ms_per_frame': round(np_s / F * 1e3, 3), 'equal': None})
        with step_limit(240, 'min_share 0 ' + name):
            free[name] = road_fit.fit_rounds_device(scans, Ts, ids, 3, 0.0, **options)

        # ---- (a), (b) the launches alone, per round
        with step_limit(300, 'the launches alone ' + name):
            sizes = [p.shape[0] for p in scans]
            offsets = np.zeros(F + 1, np.int32)
            offsets[1:] = np.cumsum(sizes)
            up = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
            points_d, offsets_d = up(np.concatenate(scans)), up(offsets)
            T_d, ids_d = up(np.asarray(Ts).reshape(F, 12)), up(np.asarray(ids, np.uint32).view(np.int32))
            mp = max(sizes)
            q, kept = hip.road_points(points_d, offsets_d, T_d, mp, o['region_q'])
            for r in range(3):
                seed = road_fit.round_seed(o['seed'], r)
                score = lambda: hip.road_score(q, offsets_d, kept, ids_d, seed, mp, o['H'], o['c2'], o['hlo2'], o['hhi2'], o['tq2'])  # noqa: E731
                count = score()
                winner, _ = hip.road_winner(count, o['min_inliers'])
                legs = [('gpp_road_score', score), ('gpp_road_winner', lambda: hip.road_winner(count, o['min_inliers'])),
                        ('gpp_road_moments', lambda: hip.road_moments(q, offsets_d, kept, ids_d, seed, winner, mp, o['H'], o['tq2']))]
                if r < 2:
                    legs.append(('gpp_road_peel_i32', lambda: hip.road_peel(q, offsets_d, kept, ids_d, seed, winner, mp, o['H'], o['tq2'])))
                for launch, fn in legs:
                    note(dict({'what': 'launch_alone', 'set': name, 'launch': launch, 'round': r}, **launch_times(fn, launches=40, skip=10)))
                if r < 2:
                    q, kept = hip.road_peel(q, offsets_d, kept, ids_d, seed, winner, mp, o['H'], o['tq2'])
            del points_d, q

    # ---- (d) what the rounds find
    share = {k: v['inliers'] / np.maximum(1, v['kept'][:, :1]) for k, v in free.items()}
    for r in range(3):
        sh = share['flat'][:, r]
        note({'what': 'flat_round', 'round': r, 'planes': int(free['flat']['valid'][:, r].sum()), 'share_median': float(np.median(sh)),
              'share_min': float(sh.min()), 'share_max': float(sh.max())})
    g = free['ramp']
    for r in range(3):
        height, angle, on_flat = [], [], 0
        for f in np.nonzero(g['valid'][:, r])[0]:
            a, b = against(g['planes'][f, r], flat_truth[f], 12.5), against(g['planes'][f, r], ramp_truth[f], 37.5)
            on_flat += a[0] <= b[0]
            height.append(min(a, b)[0]); angle.append(min(a, b)[1])
        sh = share['ramp'][:, r]
        note({'what': 'ramp_round', 'round': r, 'planes': len(height), 'on_flat': int(on_flat), 'on_ramp': len(height) - int(on_flat),
              'height_median_m': float(np.median(height)) if height else float('nan'), 'height_max_m': float(max(height)) if height else float('nan'),
              'angle_median_rad': float(np.median(angle)) if angle else float('nan'), 'angle_max_rad': float(max(angle)) if angle else float('nan'),
              'share_median': float(np.median(sh)), 'share_min': float(sh.min()), 'share_max': float(sh.max())})
    records.insert(0, {'what': 'setup', 'frames': F, 'points': args.points, 'hypotheses': args.hypotheses, 'kept_mean': kept_mean,
                       'library': hip.lib().gpp_version().decode()})
    print(json.dumps(records[0]), flush=True)

    with open(os.path.join(args.out, 'bench_road_fit_rounds.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    readme = os.path.join(args.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# Several road planes per frame: measurements\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN) + len(BEGIN)] + '\n' + readme_tables(records) + '\n' + text[text.index(END):]
        with open(readme, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
