#!/usr/bin/env python3
"""
Measures the distillation for the polled location error (utils/plane_db.py objective='location', csrc/plane_db.hip)
against the key objective of section 4.21, on one GPU, in ONE process, in the setting of tools/bench_plane_distil.py: the synthetic
val-sized dataset (`--images` label files, every object rested on a row of the shipped 100-plane database, labels with two decimals,
KITTI's P2), the 22k pool, the EVEN-numbered images distilled, the ODD-numbered ones scored.  Both objectives run in this same process:

  (a) the cost launches alone (HIP events): gpp_poll_costs_u16 (one table) against gpp_pose_costs_u16 (two tables); cost_table as a whole
  (b) the selections, K = `--planes` (10 000): gpp_plane_select against gpp_plane_select_polled; once more with K = the picks that pick,
      which gives the time per pick (one gain launch and one pick launch) without the launches behind the done flag
  (c) the held-out half: polling_ceiling (3-D / BEV AP|R40, the median location error) for the first 100 planes and the whole run of
      either objective, beside the shipped 100 / 1k / 22k files; and the polled location error of section 4.23 (polled_state_np on the
      held-out half's own two tables) for the same databases

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_plane_distil_location.jsonl and the tables of <out>/README.md between its two markers; <out> defaults to
profiles/plane_distil_location.  None of these figures is asserted anywhere: they are records.

    python tools/bench_plane_distil_location.py [--out DIR] [--images 3769] [--planes 10000]
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
from keras_retinanet_3D.utils import kitti_eval, plane_db, synthetic  # noqa: E402
from keras_retinanet_3D.utils import label_prep as L  # noqa: E402

BEGIN, END = '<!-- bench_plane_distil_location: begin -->', '<!-- bench_plane_distil_location: end -->'
SHIPPED = ('100', '1k', '22k')


def readme_tables(records):
    setup = [r for r in records if r['what'] == 'setup'][0]
    c = [r for r in records if r['what'] == 'costs'][0]
    runs = {r['objective']: r for r in records if r['what'] == 'select'}
    lines = ['`tools/bench_plane_distil_location.py`, one MI355X, one process; library `{}`.'.format(setup['library']), '',
             '{} images ({} distilled on, {} held out).  Pool: the shipped 22k database ({} planes); {} objects on the even-numbered images.'.format(
                 setup['images'], setup['even'], setup['odd'], c['pool'], c['objects']), '',
             '| step | `poll` (section 4.21) | `location` (section 4.23) | ratio |', '|---|---|---|---|',
             '| cost launch alone, {} x {} pairs (median of HIP events) | `gpp_poll_costs_u16` {:.2f} ms | `gpp_pose_costs_u16` {:.2f} ms (keys equal: {}) | {:.2f} |'.format(
                 c['objects'], c['pool'], c['poll_launch_ms'], c['pose_launch_ms'], c['keys_equal'], c['pose_launch_ms'] / c['poll_launch_ms']),
             '| `cost_table`, whole | {:.3f} s ({:.2f} GB) | {:.3f} s ({:.2f} GB) | {:.2f} |'.format(
                 c['poll_table_s'], c['table_gb'], c['pose_table_s'], 2 * c['table_gb'], c['pose_table_s'] / c['poll_table_s'])]
    a, b = runs['poll'], runs['location']
    lines += ['| selection, K = {} asked | {:.3f} s, {} picks | {:.3f} s, {} picks | |'.format(a['asked'], a['select_s'], a['count'], b['select_s'], b['count']),
              '| selection, K = its own picks (every pick picks) | {:.3f} s = {:.1f} us per pick | {:.3f} s = {:.1f} us per pick | {:.2f} per pick |'.format(
                  a['select_count_s'], a['us_per_pick'], b['select_count_s'], b['us_per_pick'], b['us_per_pick'] / a['us_per_pick']),
              '| picks shared by the two runs (first 100 / all) | | {} / {} | |'.format(b['shared_100'], b['shared_all']), '',
              'Held-out half (the odd-numbered images): `polling_ceiling`, and the polled location error of section 4.23 replayed on the held-out '
              'half\'s own tables.', '',
              '| database | planes | 3-D AP R40 E / M / H | BEV AP R40 E / M / H | location median m (`polling_ceiling`) | polled location mean / median m (4.23) | served |',
              '|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'ceiling':
            lines.append('| {} | {} | {} | {} | {:.3f} | {:.3f} / {:.3f} | {} of {} |'.format(
                r['database'], r['planes'], ' / '.join('%.2f' % v for v in r['ap_3d']), ' / '.join('%.2f' % v for v in r['ap_bev']),
                r['location_error_median_m'], r['polled']['mean_location_m'], r['polled']['median_location_m'], r['polled']['served'], r['polled']['objects']))
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plane_distil_location'))
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

        def read_half(h):
            ld, cd = halves[h]
            names = sorted(os.listdir(ld))
            return [kitti_eval.read_label_file(os.path.join(ld, f)) for f in names], [L.read_calibration(os.path.join(cd, f)) for f in names]

        # ---- (a) the cost tables of the even half, both forms
        pool = synthetic.load_plane_database('22k')
        K = min(args.planes, pool.shape[0])
        labels_list, P_list = read_half('even')
        with step_limit(240, 'the cost tables'):
            plane_db.cost_table(labels_list[:8], P_list[:8], pool)                       # (first launches: code objects load)
            plane_db.cost_table(labels_list[:8], P_list[:8], pool, errors=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table, M = plane_db.cost_table(labels_list, P_list, pool)
            torch.cuda.synchronize()
            poll_table_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            keys, errs, _ = plane_db.cost_table(labels_list, P_list, pool, errors=True)
            torch.cuda.synchronize()
            pose_table_s = time.perf_counter() - t0
            O = int(table.shape[0])
            keys_equal = bool(torch.equal(keys, table))
        with step_limit(240, 'the cost launches alone'):
            A = max(g.shape[0] for g in labels_list)
            labels_d, counts_d, P_d, trig_d = L._upload(labels_list, P_list, A)
            pinv_d = torch.as_tensor(np.stack([np.linalg.pinv(P) for P in P_list]).astype(np.float32)).cuda()
            _, (boxes, dims, _, _, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, L.CAR, True, True)
            rows = torch.nonzero(orient.reshape(-1) >= 0).reshape(-1).to(torch.int32)
            want_d = torch.as_tensor(np.ascontiguousarray(kitti_eval.pack_labels(labels_list, A)[0][..., 11:14].astype(np.float32))).cuda()
            planes_d = torch.as_tensor(pool.astype(np.float32)).cuda()
            again, again_e = torch.empty_like(table), torch.empty_like(table)
            poll = launch_times(lambda: hip.poll_costs(boxes, dims, orient, pinv_d, planes_d, again, rows, 0), launches=6, skip=1)
            pose = launch_times(lambda: hip.pose_costs(boxes, dims, orient, pinv_d, want_d, planes_d, again, again_e, rows, 0), launches=6, skip=1)
            del again, again_e
        note({'what': 'costs', 'pool': M, 'objects': O, 'table_gb': round(O * int(table.shape[1]) * 2 / 1e9, 3), 'poll_table_s': round(poll_table_s, 4),
              'pose_table_s': round(pose_table_s, 4), 'poll_launch_ms': round(poll['median_us'] / 1e3, 3), 'pose_launch_ms': round(pose['median_us'] / 1e3, 3),
              'keys_equal': keys_equal})

        # ---- (b) the two selections
        picked = {}
        for objective, run in (('poll', lambda n: plane_db.select(table, M, n)), ('location', lambda n: plane_db.select_polled(keys, errs, M, n))):
            with step_limit(600, 'the selection ' + objective):
                run(8)                                                                   # (first launches)
                t0 = time.perf_counter()
                got = run(K)
                select_s = time.perf_counter() - t0
                t0 = time.perf_counter()
                run(max(1, got['count']))                                                # the picks that pick, without the launches behind the done flag
                select_count_s = time.perf_counter() - t0
            picked[objective] = got
            rec = {'what': 'select', 'objective': objective, 'asked': K, 'count': got['count'], 'select_s': round(select_s, 4),
                   'select_count_s': round(select_count_s, 4), 'us_per_pick': round(select_count_s / max(1, got['count']) * 1e6, 2),
                   'trace_0': int(got['trace'][0]), 'trace_end': int(got['trace'][-1])}
            if objective == 'location':
                a, b = picked['poll'], got
                rec['shared_100'] = len(set(a['chosen'][:100].tolist()) & set(b['chosen'][:100].tolist()) - {-1})
                rec['shared_all'] = len(set(a['chosen'][:a['count']].tolist()) & set(b['chosen'][:b['count']].tolist()))
                rec.update(plane_db.location_summary(got['cur']))
            note(rec)
        del table, keys, errs

        # ---- (c) the held-out half
        ld, cd = halves['odd']
        labels_list, P_list = read_half('odd')
        with step_limit(240, 'the held-out tables'):
            keys, errs, _ = plane_db.cost_table(labels_list, P_list, pool, errors=True)
            torch.cuda.synchronize()
        databases = [('shipped ' + n, synthetic.load_plane_database(n), None) for n in SHIPPED]
        for objective in ('poll', 'location'):
            got = picked[objective]
            for n in sorted({min(100, got['count']), got['count']}):
                databases.append(('{} {}'.format(objective, n), pool[got['chosen'][:n]], got['chosen'][:n]))
        for name, planes, order in databases:
            with step_limit(240, 'polling_ceiling ' + name):
                result = L.polling_ceiling(ld, cd, planes)
                if order is None:                                                        # a shipped file: its own two tables
                    k2, e2, m2 = plane_db.cost_table(labels_list, P_list, planes, errors=True)
                    order, hk, he = np.arange(m2), k2[:, :m2].cpu().numpy().view(np.uint16), e2[:, :m2].cpu().numpy().view(np.uint16)
                    del k2, e2
                else:
                    cols = torch.as_tensor(np.asarray(order, np.int64)).cuda()
                    hk, he = keys[:, cols].cpu().numpy().view(np.uint16), errs[:, cols].cpu().numpy().view(np.uint16)
                    order = np.arange(len(order))
                _, cur = plane_db.polled_state_np(hk, he, order)
            note({'what': 'ceiling', 'database': name, 'planes': int(planes.shape[0]),
                  'ap_3d': [round(result[('3d', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                  'ap_bev': [round(result[('bev', d)]['ap_r40'], 4) for d in kitti_eval.DIFFICULTIES],
                  'location_error_median_m': result['summary']['location_error_median_m'], 'polled': plane_db.location_summary(cur)})

    with open(os.path.join(args.out, 'bench_plane_distil_location.jsonl'), 'w') as f:
        for rec in records:
            f.write(json.dumps(rec) + '\n')
    readme = os.path.join(args.out, 'README.md')
    text = open(readme).read() if os.path.isfile(readme) else '# Distilling for the polled location error: measurements\n\n{}\n{}\n'.format(BEGIN, END)
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN) + len(BEGIN)] + '\n' + readme_tables(records) + '\n' + text[text.index(END):]
        with open(readme, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
