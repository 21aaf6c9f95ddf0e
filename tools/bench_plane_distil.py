#!/usr/bin/env python3
"""
Measures the plane distillation (utils/plane_db.py, csrc/plane_db.hip) on one GPU, in ONE process, on the synthetic
val-sized dataset of tools/bench_label_prep.py (`--images` label files, every object rested on a row of the shipped 100-plane database,
labels with two decimals, KITTI's P2):

  (a) distil K = `--planes` (10 000) planes from the 22k pool on the EVEN-numbered images: seconds of the cost table, of the cost launch
      alone (HIP events), of the selection loop; NumPy's select_np on a corner of the table that finishes, and its extrapolation to the
      whole table (per pick the work is O x M: the extrapolation scales the measured pick by that ratio) -- reported as an extrapolation
  (b) polling_ceiling on the ODD-numbered images for the shipped 100 / 1k / 22k and the distilled 100 / 1k / 10k prefixes of that ONE run
      (those the run reaches, and the whole run):
      3-D and BEV AP|R40, the median location error
  (c) HIP events around gpp_poll_f32 alone on the odd half as one chunk, at each database size

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_plane_distil.jsonl and the tables of <out>/README.md between its two markers; <out> defaults to profiles/plane_distil.
None of these figures is asserted anywhere: they are records.

    python tools/bench_plane_distil.py [--out DIR] [--images 3769] [--planes 10000]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_kitti_eval import launch_times, step_limit, write_dataset  # noqa: E402
from bench_label_prep import rest_on_planes  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import gpp_utils, kitti_eval, plane_db, synthetic  # noqa: E402
from keras_retinanet_3D.utils import label_prep as L  # noqa: E402

BEGIN, END = '<!-- bench_plane_distil: begin -->', '<!-- bench_plane_distil: end -->'
SHIPPED = ('100', '1k', '22k')
NP_CORNER = (2000, 2000, 20)                                # rows, planes and picks of the select_np leg


def readme_tables(records):
    setup = [r for r in records if r['what'] == 'setup'][0]
    d = [r for r in records if r['what'] == 'distil'][0]
    h = [r for r in records if r['what'] == 'select_np'][0]
    lines = ['`tools/bench_plane_distil.py`, one MI355X, one process; library `{}`.'.format(setup['library']), '',
             '{} images ({} distilled on, {} held out).  Pool: the shipped 22k database ({} planes); {} objects on the even-numbered images; '
             'K = {} asked, {} picked (no plane of the pool lowers the objective after that: the distilled 1k / 10k ARE this run).'.format(setup['images'], setup['even'], setup['odd'], d['pool'], d['objects'], d['asked'], d['count']), '',
             '| step | time |', '|---|---|',
             '| cost table, whole (`cost_table`: upload, `gpp_label_prep_f64`, row lists, `gpp_poll_costs_u16`) | {:.3f} s |'.format(d['cost_table_s']),
             '| `gpp_poll_costs_u16` launch alone ({} x {} pairs, {:.2f} GB written) | {:.2f} ms |'.format(d['objects'], d['pool'], d['table_gb'], d['cost_launch_ms']),
             '| `gpp_plane_select`, K = {} ({} launches, the run ends after {} picks) | {:.3f} s |'.format(d['asked'], 2 * d['asked'] + 1, d['count'], d['select_s']),
             '| `gpp_plane_select`, K = {} (every pick picks) | {:.3f} s = {:.1f} us per pick |'.format(d['count'], d['select_count_s'], d['select_count_s'] / max(1, d['count']) * 1e6),
             '| `select_np` on a {} x {} corner, {} picks (equal to the kernel: {}) | {:.3f} s = {:.1f} ms per pick |'.format(
                 h['rows'], h['planes'], h['picks'], h['equal'], h['seconds'], h['seconds'] / h['picks'] * 1e3),
             '| `select_np` on the whole table, EXTRAPOLATED (per pick x {:.0f}, x {} picks) | {:.0f} s |'.format(h['scale'], d['asked'], h['extrapolated_s']), '',
             '| prefix | objective per object | six votes | median residual m |', '|---|---|---|---|']
    for n, s in sorted((int(k), v) for k, v in d['prefixes'].items()):
        lines.append('| {} | {:.1f} | {:.2%} | {:.4f} |'.format(n, s['objective'] / d['objects'], s['six_vote_share'], s['median_residual_m']))
    lines += ['', 'Held-out half (`polling_ceiling` on the odd-numbered images):', '',
              '| database | planes | 3-D AP R40 E / M / H | BEV AP R40 E / M / H | location median m | `gpp_poll_f32` launch ms (median) |', '|---|---|---|---|---|---|']
    launch = {r['planes']: r for r in records if r['what'] == 'poll_launch'}
    for r in records:
        if r['what'] == 'ceiling':
            lines.append('| {} | {} | {} | {} | {:.3f} | {:.3f} |'.format(
                r['database'], r['planes'], ' / '.join('%.2f' % v for v in r['ap_3d']), ' / '.join('%.2f' % v for v in r['ap_bev']),
                r['location_error_median_m'], launch[r['planes']]['median_us'] / 1e3))
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plane_distil'))
    ap.add_argument('--images', type=int, default=3769)
    ap.add_argument('--planes', type=int, default=10000)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records = []

    def note(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    with tempfile.TemporaryDirectory() as root:
        label_dir, calib_dir = os.path.join(root, 'label_2'), os.path.join(root, 'calib')
        halves = {h: (os.path.join(root, h, 'label_2'), os.path.join(root, h, 'calib')) for h in ('even', 'odd')}
        for d in [label_dir, calib_dir] + [p for pair in halves.values() for p in pair]:
            os.makedirs(d)
        with step_limit(420, 'the dataset'):
            write_dataset(label_dir, args.images)
            rest_on_planes(label_dir, {calib_dir: synthetic.KITTI_LIKE_P2.copy()}, synthetic.load_plane_database('100'))
            files = sorted(os.listdir(label_dir))
            for i, f in enumerate(files):
                ld, cd = halves['odd' if i % 2 else 'even']
                shutil.copy(os.path.join(label_dir, f), os.path.join(ld, f))
                shutil.copy(os.path.join(calib_dir, f), os.path.join(cd, f))
            note({'what': 'setup', 'images': args.images, 'even': len(os.listdir(halves['even'][0])), 'odd': len(os.listdir(halves['odd'][0])),
                  'library': hip.lib().gpp_version().decode()})

        # ---- (a) the distillation on the even half
        pool = synthetic.load_plane_database('22k')
        K = min(args.planes, pool.shape[0])
        ld, cd = halves['even']
        even = sorted(os.listdir(ld))
        labels_list = [kitti_eval.read_label_file(os.path.join(ld, f)) for f in even]
        P_list = [L.read_calibration(os.path.join(cd, f)) for f in even]
        with step_limit(240, 'the cost table'):
            plane_db.cost_table(labels_list[:8], P_list[:8], pool)                       # (first launches: code objects load)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table, M = plane_db.cost_table(labels_list, P_list, pool)
            torch.cuda.synchronize()
            cost_table_s = time.perf_counter() - t0
            O = int(table.shape[0])
        with step_limit(240, 'the cost launch alone'):
            A = max(g.shape[0] for g in labels_list)
            labels_d, counts_d, P_d, trig_d = L._upload(labels_list, P_list, A)
            pinv_d = torch.as_tensor(np.stack([np.linalg.pinv(P) for P in P_list]).astype(np.float32)).cuda()
            _, (boxes, dims, _, _, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, L.CAR, True, True)
            rows = torch.nonzero(orient.reshape(-1) >= 0).reshape(-1).to(torch.int32)
            planes_d = torch.as_tensor(pool.astype(np.float32)).cuda()
            again = torch.empty_like(table)
            cost = launch_times(lambda: hip.poll_costs(boxes, dims, orient, pinv_d, planes_d, again, rows, 0), launches=6, skip=1)
            same_table = bool(torch.equal(again[:, :M], table[:, :M]))
            del again
        with step_limit(600, 'the selection'):
            t0 = time.perf_counter()
            picked = plane_db.select(table, M, K)
            select_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            plane_db.select(table, M, max(1, picked['count']))                           # the picks that pick, without the launches behind the done flag
            select_count_s = time.perf_counter() - t0
        prefixes = {}
        with step_limit(300, 'the prefixes'):
            for n in sorted({n for n in (100, 1000, K) if n <= picked['count']} | {picked['count']}):
                short = picked if n == picked['count'] else plane_db.select(table, M, n)
                assert np.array_equal(short['chosen'][:n], picked['chosen'][:n])
                prefixes[n] = dict(plane_db.best_summary(short['best']), objective=int(picked['trace'][n]))
        note({'what': 'distil', 'pool': M, 'objects': O, 'asked': K, 'count': picked['count'], 'cost_table_s': round(cost_table_s, 4),
              'cost_launch_ms': round(cost['median_us'] / 1e3, 3), 'cost_launch_equal': same_table, 'table_gb': round(O * int(table.shape[1]) * 2 / 1e9, 3),
              'select_s': round(select_s, 4), 'select_count_s': round(select_count_s, 4), 'prefixes': prefixes, 'trace_0': int(picked['trace'][0]), 'trace_end': int(picked['trace'][-1])})
        with step_limit(420, 'select_np'):
            r, c, k = min(NP_CORNER[0], O), min(NP_CORNER[1], M), NP_CORNER[2]
            corner = table[:r, :c].cpu().numpy().view(np.uint16)
            t0 = time.perf_counter()
            host = plane_db.select_np(corner, k)
            seconds = time.perf_counter() - t0
            dev = plane_db.select(table[:r, :hip.table_pitch(c)].contiguous(), c, k)
            equal = all(np.array_equal(host[n], dev[n]) for n in ('chosen', 'trace', 'best')) and host['count'] == dev['count']
            scale = (O * M) / float(r * c)
            note({'what': 'select_np', 'rows': r, 'planes': c, 'picks': k, 'seconds': round(seconds, 4), 'equal': bool(equal), 'scale': round(scale, 2),
                  'extrapolated_s': round(seconds / k * scale * K, 1)})
        del table
        distilled = pool[picked['chosen'][:picked['count']]]
        plane_db.write_database(os.path.join(root, 'distilled.mat'), distilled)
        assert np.array_equal(L._load_planes(os.path.join(root, 'distilled.mat')), distilled.astype(np.float32))

        # ---- (b) the held-out half
        ld, cd = halves['odd']
        databases = [('shipped ' + n, synthetic.load_plane_database(n)) for n in SHIPPED]
        databases += [('distilled {}'.format(n), distilled[:n]) for n in sorted({n for n in (100, 1000, K) if n <= distilled.shape[0]} | {distilled.shape[0]})]
        for name, planes in databases:
            with step_limit(240, 'polling_ceiling ' + name):
                result = L.polling_ceiling(ld, cd, planes)
            note({'what': 'ceiling', 'database': name, 'planes': int(planes.shape[0]),
                  'ap_3d': [round(result[('3d', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                  'ap_bev': [round(result[('bev', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                  'location_error_median_m': result['summary']['location_error_median_m'], 'summary': result['summary']})

        # ---- (c) the polling launch alone on the odd half as one chunk
        with step_limit(240, 'the polling launches'):
            odd = sorted(os.listdir(ld))
            labels_list = [kitti_eval.read_label_file(os.path.join(ld, f)) for f in odd]
            P_list = [L.read_calibration(os.path.join(cd, f)) for f in odd]
            A = max(g.shape[0] for g in labels_list)
            labels_d, counts_d, P_d, trig_d = L._upload(labels_list, P_list, A)
            pinv_d = torch.as_tensor(np.stack([np.linalg.pinv(P) for P in P_list]).astype(np.float32)).cuda()
            _, (boxes, dims, _, _, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, L.CAR, True, True)
            for n in sorted({int(p.shape[0]) for _, p in databases}):
                planes_d = torch.as_tensor([p for _, p in databases if p.shape[0] == n][0].astype(np.float32)).cuda()
                note(dict({'what': 'poll_launch', 'planes': n, 'B': len(odd), 'A': A},
                          **launch_times(lambda: gpp_utils.fit_road_planes(boxes, dims, orient, pinv_d, planes_d), launches=30, skip=5)))

    with open(os.path.join(args.out, 'bench_plane_distil.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    readme = os.path.join(args.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# Plane-database distillation: measurements\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN) + len(BEGIN)] + '\n' + readme_tables(records) + '\n' + text[text.index(END):]
        with open(readme, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
