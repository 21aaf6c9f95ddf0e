#!/usr/bin/env python3
"""
Measures the per-frame road-plane fit (utils/road_fit.py, csrc/road_fit.hip) on one GPU, in ONE process, on `--frames`
(64) synthetic scans of `--points` (120 000) points each: a disc of 62 m around the sensor, so that about 20 000 points fall into the
default region; per frame a road of its own (height 1.5 .. 1.8 m, slopes within +-0.03) with 2 cm Gaussian noise, 30 % of the points
lifted by up to 2 m (clutter), a velodyne -> camera matrix with the digits of a KITTI calibration line.  H = `--hypotheses` (1 024).

  (a) HIP events around each of the four launches alone, the batch as one chunk; the score launch's share of the board's float64 vector
      rate: the kernel carries its integers in float64 -- per (kept point, valid hypothesis) pair three v_fma_f64, one v_mul_f64 and one
      v_cmp -- so the bound is 5 float64 instructions per pair at 78.6 TFLOP/s / 2 (one fused multiply-add counts two operations)
  (b) fit_device on the batch (upload, four launches, fetch, solve_moments) and fit_pool on the same scans written as files (reading
      included), seconds per frame; fit_np on the same frames in the same process (the comparison, not a bar); device == host is checked
  (c) the fitted plane against the truth on these noisy clouds: the height error at the region's centre (x = 0, z = 25 m) and the angle
      between the normals -- recorded, not asserted: there is no reference to set a bar against; the exact cases of the tests pin the code

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_road_fit.jsonl and the tables of <out>/README.md between its two markers; <out> defaults to profiles/road_fit.
None of these figures is asserted anywhere: they are records.

    python tools/bench_road_fit.py [--out DIR] [--frames 64] [--points 120000] [--hypotheses 1024]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_kitti_eval import launch_times, step_limit  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import road_fit  # noqa: E402

BEGIN, END = '<!-- bench_road_fit: begin -->', '<!-- bench_road_fit: end -->'
F64_INSTR_PER_S = 78.6e12 / 2.0                             # float64 vector instructions per second: the board's 78.6 TFLOP/s counts an FMA as two
INSTR_PER_PAIR = 5                                          # 3 v_fma_f64 + v_mul_f64 + v_cmp_le_f64
VELO_TO_CAM = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                        [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]])


def synthetic_scan(rng, n):
    """ (scan (n, 4) float32, truth (4,) canonical plane): see the module docstring """
    r, phi = 62.0 * np.sqrt(rng.random(n)), rng.uniform(0.0, 2.0 * np.pi, n)
    x, z = r * np.sin(phi), r * np.cos(phi)
    h, a, c = rng.uniform(1.5, 1.8), rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03)
    y = h + a * x + c * z + rng.normal(0.0, 0.02, n)
    lifted = rng.random(n) < 0.3
    y[lifted] -= rng.uniform(0.0, 2.0, int(lifted.sum()))
    cam = np.stack([x, y, z], axis=1)
    velo = (cam - VELO_TO_CAM[:, 3]) @ np.linalg.inv(VELO_TO_CAM[:, :3]).T
    scan = np.concatenate([velo, rng.random((n, 1))], axis=1).astype(np.float32)
    return scan, np.array([a, -1.0, c, h]) / np.sqrt(a * a + 1.0 + c * c)


def plane_errors(planes, truths):
    """ per frame |height difference| at (x, z) = (0, 25 m) in metres and the angle between the normals in radians """
    height = lambda p: -(p[:, 2] * 25.0 + p[:, 3]) / p[:, 1]  # noqa: E731
    cos = np.clip((planes[:, :3] * truths[:, :3]).sum(axis=1), -1.0, 1.0)
    return np.abs(height(planes) - height(truths)), np.arccos(cos)


def readme_tables(records):
    s = [r for r in records if r['what'] == 'setup'][0]
    sc = [r for r in records if r['what'] == 'score_share'][0]
    w = [r for r in records if r['what'] == 'wall'][0]
    e = [r for r in records if r['what'] == 'noisy_clouds'][0]
    lines = ['`tools/bench_road_fit.py`, one MI355X, one process; library `{}`.'.format(s['library']), '',
             '{} synthetic frames of {} points, {:.0f} kept per frame on average (region 20 / 8 / 50 m), H = {}; {} of {} frames gave a plane; '
             'the device result {} the NumPy form\'s.'.format(s['frames'], s['points'], s['kept_mean'], s['hypotheses'], s['valid'], s['frames'],
                                                               'EQUALS' if w['device_equals_host'] else 'DIFFERS FROM'), '',
             '| launch alone (HIP events, the {} frames as one chunk) | median us | min us |'.format(s['frames']), '|---|---|---|']
    for r in records:
        if r['what'] == 'launch_alone':
            lines.append('| `{}` | {} | {} |'.format(r['launch'], r['median_us'], r['min_us']))
    lines += ['', 'The score launch carries its integers in float64: {:.3e} (kept point, valid hypothesis) pairs x {} float64 vector instructions '
              '(3 `v_fma_f64`, `v_mul_f64`, `v_cmp_le_f64`) = {:.3e} instructions; at the board\'s float64 vector rate (78.6 TFLOP/s, an FMA two operations: '
              '{:.3e} instructions/s) the least time is {:.1f} us; the launch\'s median is {:.1f} us: **{:.1%} of the float64 vector rate**.'.format(
                  sc['pairs'], INSTR_PER_PAIR, sc['pairs'] * INSTR_PER_PAIR, F64_INSTR_PER_S, sc['bound_us'], sc['median_us'], sc['share']), '',
              '| whole fit | seconds | per frame |', '|---|---|---|',
              '| `fit_device` (upload, four launches, fetch, `solve_moments`) | {:.3f} | {:.2f} ms |'.format(w['fit_device_s'], w['fit_device_s'] / s['frames'] * 1e3),
              '| `fit_pool(device=True)` on the scans as files (reading included) | {:.3f} | {:.2f} ms |'.format(w['fit_pool_s'], w['fit_pool_s'] / s['frames'] * 1e3),
              '| `fit_np` on the same frames, same process (the comparison, not a bar) | {:.3f} | {:.2f} ms |'.format(w['fit_np_s'], w['fit_np_s'] / s['frames'] * 1e3), '',
              'Noisy clouds (2 cm Gaussian noise, 30 % clutter up to 2 m above the road), fitted plane against the truth over the {} valid frames -- '
              'recorded, not asserted:'.format(e['frames']), '',
              '| | median | max |', '|---|---|---|',
              '| height error at x = 0, z = 25 m | {:.2f} mm | {:.2f} mm |'.format(e['height_median_m'] * 1e3, e['height_max_m'] * 1e3),
              '| angle between the normals | {:.2e} rad | {:.2e} rad |'.format(e['angle_median_rad'], e['angle_max_rad']),
              '| RMS distance of the inliers (`rms`) | {:.2f} mm | {:.2f} mm |'.format(e['rms_median_m'] * 1e3, e['rms_max_m'] * 1e3),
              '| inliers | {:.0f} | {:.0f} |'.format(e['inliers_median'], e['inliers_max'])]
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'road_fit'))
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
    scans, truths = [m[0] for m in made], np.stack([m[1] for m in made])
    Ts, ids = [VELO_TO_CAM] * args.frames, list(range(args.frames))
    options = dict(hypotheses=args.hypotheses)
    o = road_fit.resolve_options(**options)

    # ---- (b) first: it also warms every launch up
    with step_limit(240, 'fit_device'):
        road_fit.fit_device(scans[:2], Ts[:2], ids[:2], **options)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = road_fit.fit_device(scans, Ts, ids, **options)
        fit_device_s = time.perf_counter() - t0
    with step_limit(420, 'fit_np'):
        t0 = time.perf_counter()
        want = road_fit.fit_np(scans, Ts, ids, **options)
        fit_np_s = time.perf_counter() - t0
    equal = all(got[k].tobytes() == want[k].tobytes() for k in want)
    with tempfile.TemporaryDirectory() as root, step_limit(300, 'fit_pool'):
        velo, calib = os.path.join(root, 'velodyne'), os.path.join(root, 'calib')
        os.makedirs(velo), os.makedirs(calib)
        for i, p in enumerate(scans):
            p.tofile(os.path.join(velo, '%06d.bin' % i))
            with open(os.path.join(calib, '%06d.txt' % i), 'w') as f:
                f.write('R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: ' + ' '.join(repr(float(v)) for v in VELO_TO_CAM.ravel()) + '\n')
        t0 = time.perf_counter()
        pool = road_fit.fit_pool(velo, calib, **options)
        fit_pool_s = time.perf_counter() - t0
        equal = equal and pool['record']['planes'].tobytes() == want['planes'].tobytes()
    note({'what': 'setup', 'frames': args.frames, 'points': args.points, 'hypotheses': args.hypotheses, 'kept_mean': float(np.mean(got['kept'])),
          'valid': int(got['valid'].sum()), 'library': hip.lib().gpp_version().decode()})
    note({'what': 'wall', 'fit_device_s': round(fit_device_s, 4), 'fit_pool_s': round(fit_pool_s, 4), 'fit_np_s': round(fit_np_s, 4),
          'device_equals_host': bool(equal)})

    # ---- (a) the launches alone
    with step_limit(240, 'the launches alone'):
        sizes = [p.shape[0] for p in scans]
        offsets = np.zeros(args.frames + 1, np.int32)
        offsets[1:] = np.cumsum(sizes)
        up = lambda a: torch.as_tensor(a).to(dev)  # noqa: E731
        points_d, offsets_d = up(np.concatenate(scans)), up(offsets)
        T_d, ids_d = up(np.asarray(Ts).reshape(args.frames, 12)), up(np.asarray(ids, np.uint32).view(np.int32))
        mp = max(sizes)
        q, kept = hip.road_points(points_d, offsets_d, T_d, mp, o['region_q'])
        count = hip.road_score(q, offsets_d, kept, ids_d, o['seed'], mp, o['H'], o['c2'], o['hlo2'], o['hhi2'], o['tq2'])
        winner, _ = hip.road_winner(count, o['min_inliers'])
        legs = (('gpp_road_points_i32', lambda: hip.road_points(points_d, offsets_d, T_d, mp, o['region_q'])),
                ('gpp_road_score', lambda: hip.road_score(q, offsets_d, kept, ids_d, o['seed'], mp, o['H'], o['c2'], o['hlo2'], o['hhi2'], o['tq2'])),
                ('gpp_road_winner', lambda: hip.road_winner(count, o['min_inliers'])),
                ('gpp_road_moments', lambda: hip.road_moments(q, offsets_d, kept, ids_d, o['seed'], winner, mp, o['H'], o['tq2'])))
        times = {}
        for name, fn in legs:
            times[name] = launch_times(fn, launches=40, skip=10)
            note(dict({'what': 'launch_alone', 'launch': name}, **times[name]))
        pairs = int((kept.cpu().numpy().astype(np.int64) * (count.cpu().numpy() >= 0).sum(axis=1)).sum())
        bound_us = pairs * INSTR_PER_PAIR / F64_INSTR_PER_S * 1e6
        note({'what': 'score_share', 'pairs': pairs, 'bound_us': round(bound_us, 2), 'median_us': times['gpp_road_score']['median_us'],
              'share': round(bound_us / times['gpp_road_score']['median_us'], 4), 'form': 'float64'})

    # ---- (c) the noisy clouds against the truth
    ok = got['valid']
    height, angle = plane_errors(got['planes'][ok], truths[ok])
    note({'what': 'noisy_clouds', 'frames': int(ok.sum()), 'height_median_m': float(np.median(height)), 'height_max_m': float(height.max()),
          'angle_median_rad': float(np.median(angle)), 'angle_max_rad': float(angle.max()), 'rms_median_m': float(np.median(got['rms'][ok])),
          'rms_max_m': float(got['rms'][ok].max()), 'inliers_median': float(np.median(got['inliers'][ok])), 'inliers_max': float(got['inliers'][ok].max())})

    with open(os.path.join(args.out, 'bench_road_fit.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    readme = os.path.join(args.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# Road-plane fit: measurements\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN) + len(BEGIN)] + '\n' + readme_tables(records) + '\n' + text[text.index(END):]
        with open(readme, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
