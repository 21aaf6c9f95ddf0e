#!/usr/bin/env python3
"""
Measures the identity scores (csrc/idf1_eval.hip, utils/idf1_eval.py) on one GPU, in ONE process.

  1. `kitti`, the synthetic dataset of KITTI tracking's training size that tools/bench_mot_eval.py builds (21 sequences, about 8 000
     frames): the two launches -- gpp_idf1_count, gpp_idf1_assign -- on resident inputs, HIP events around each, median of 50, with
     gpp_mot_assign and gpp_hota_potential beside them for scale; the whole evaluate_sequences(device=True, idf1=True) against the same
     call without it (median of 7); the NumPy form on the same codes (once); per sequence scipy's linear_sum_assignment on the metric's
     (G + T) x (G + T) formulation, and whether its IDFN and IDFP are the kernel's.
  2. written tables, gpp_idf1_assign alone (median of 7; of 3 above 10^6 cells): 21 sparse tables of 100 x 300 in one launch -- the sides
     the real KITTI sequences have --, and dense tables of counts in {0, 1, 2}, where ties rule, of 256 x 256, 1024 x 1024 and
     1024 x 4096; scipy on the same rectangular matrix beside each, and whether the totals agree.

    python tools/bench_idf1.py --steps-only     no GPU: counts the dependent steps of every written table with the NumPy form (minutes)
                                                 and writes <out>/steps.json; a later run on the GPU divides its times by them

Every GPU step runs under a time limit of its own (SIGALRM: the process ends there, nothing more is started).  Writes
<out>/bench_idf1.jsonl (one JSON record per measurement) and <out>/tables.md; <out> defaults to profiles/idf1.

    python tools/bench_idf1.py [--out DIR] [--frames 8000] [--steps-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_mot_eval import kitti_sized, median_us, step_limit  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.utils import hota_eval as H  # noqa: E402
from keras_retinanet_3D.utils import idf1_eval as I  # noqa: E402
from keras_retinanet_3D.utils import kitti_eval  # noqa: E402
from keras_retinanet_3D.utils import mot_eval as M  # noqa: E402
from keras_retinanet_3D.utils import pair_tables as PT  # noqa: E402

SCALE = I.SCALE


# ---------------------------------------------------------------------------------------------------- the written tables
def sparse(seed, G, T, per_row=4, pool=None):
    rng = np.random.default_rng(seed)
    C = np.zeros((G, T), np.int32)
    for g in range(G):
        C[g, rng.integers(0, T if pool is None else pool, per_row)] = rng.integers(1, 40, per_row)
    return C


def dense(seed, G, T):
    return np.random.default_rng(seed).integers(0, 3, (G, T)).astype(np.int32)


def written_tables():
    """ [(name, [tables of one launch])] """
    return [('21 x sparse 100 x 300', [sparse(100 + s, 100, 300, per_row=8, pool=120) for s in range(21)]),
            ('dense 256 x 256', [dense(1, 256, 256)]), ('dense 1024 x 1024', [dense(2, 1024, 1024)]), ('dense 1024 x 4096', [dense(3, 1024, 4096)])]


def count_steps(out):
    steps = {}
    for name, tables in written_tables():
        t0, total = time.perf_counter(), []
        for C in tables:
            stats = {}
            I.assign_table_np(C, stats)
            total.append(stats['steps'])
        steps[name] = {'steps': total, 'numpy_s': round(time.perf_counter() - t0, 2)}
        print(name, steps[name]['numpy_s'], 's', sum(total), 'steps, the longest table', max(total))
    with open(os.path.join(out, 'steps.json'), 'w') as f:
        json.dump(steps, f, indent=1)


def rectangular_total(C):
    from scipy.optimize import linear_sum_assignment
    cost = np.full((C.shape[0], max(C.shape)), SCALE, np.int64)
    cost[:, :C.shape[1]] -= C
    ri, ci = linear_sum_assignment(cost)
    return int(cost[ri, ci].sum())


def definition_counts(C, gc, tc):
    """ the metric's (G + T) x (G + T) formulation -> (IDFN, IDFP) """
    from scipy.optimize import linear_sum_assignment
    C, gc, tc = np.asarray(C, np.float64), np.asarray(gc, np.float64), np.asarray(tc, np.float64)
    G, T = C.shape
    fn, fp = np.zeros((G + T, G + T)), np.zeros((G + T, G + T))
    fp[G:, :T] = fn[:G, T:] = 1e10
    for g in range(G):
        fn[g, :T], fn[g, T + g] = gc[g] - C[g], gc[g]
    for t in range(T):
        fp[:G, t], fp[G + t, t] = tc[t] - C[:, t], tc[t]
    ri, ci = linear_sum_assignment(fn + fp)
    return int(round(fn[ri, ci].sum())), int(round(fp[ri, ci].sum()))


def tables_on_device(records, steps):
    dev = hip.require_device()
    for name, tables in written_tables():
        seq_tab, _, cells, vecs = PT.tables([0] * (len(tables) + 1), [C.shape[0] for C in tables], [C.shape[1] for C in tables])
        with step_limit(240, name):
            workspace = hip.idf1_workspace(cells, vecs, 0, len(tables), dev)
            table, cnt = hip.idf1_tables(workspace, cells, vecs)
            for C, (cell_base, n_gt, n_trk, vec_base, _, _) in zip(tables, seq_tab.tolist()):
                table[cell_base:cell_base + n_gt * n_trk] = torch.as_tensor(C.reshape(-1)).to(dev)
            tab = seq_tab.reshape(-1)
            med, low = median_us(lambda: hip.idf1_assign(tab, cells, vecs, workspace), n=3 if cells > 1000000 else 7, warm=1)
            seq = hip.idf1_assign(tab, cells, vecs, workspace)[1].cpu().numpy()
        t0 = time.perf_counter()
        totals = [rectangular_total(C) for C in tables]
        t_scipy = time.perf_counter() - t0
        n_steps = steps.get(name, {}).get('steps')
        longest = max(n_steps) if n_steps else None      # (the sequences of a launch run side by side: the longest one is the launch)
        records.append({'what': 'table', 'tables': name, 'cells': cells, 'gpp_idf1_assign_median_us': med, 'min_us': low,
                        'scipy_rectangular_ms': round(t_scipy * 1e3, 2), 'totals_equal': bool(seq[:, 5].tolist() == totals),
                        'idtp': int(seq[:, 0].sum()), 'steps_longest_table': longest,
                        'us_per_step': round(med / longest, 3) if longest else None,
                        'numpy_s': steps.get(name, {}).get('numpy_s')})


# ---------------------------------------------------------------------------------------------------- the KITTI-sized set
def kitti(records, frames):
    labels, tracks = kitti_sized(frames)
    params = M.check_params()
    packed = M.pack_sequences(labels, tracks)
    dev = hip.require_device()
    N, A, D = packed.labels.shape[0], packed.labels.shape[1], packed.rows.shape[1]
    rows, ids = torch.as_tensor(packed.rows).to(dev), torch.as_tensor(packed.ids).to(dev)
    lab, counts = torch.as_tensor(packed.labels).to(dev), torch.as_tensor(packed.label_counts).to(dev)
    traj = torch.as_tensor(packed.traj).to(dev)
    prm = hip.MotParams(0, 0, params['min_overlap'], params['max_occlusion'], params['max_truncation'], params['min_height'])
    assert kitti_eval.chunk_images(D, A) >= N, 'one chunk'
    with step_limit(180, 'kitti: launches alone'):
        overlaps = hip.kitti_overlaps(rows, lab, counts)
        _, lout, rout, _ = hip.mot_assign(overlaps, lab, counts, rows, ids, prm)
        geo = PT.Geometry(packed, params, rows, ids, traj)
        hota = H.DeviceRun(geo, N, dev)
        run = I.DeviceRun(geo, N, dev)
        tab = geo.frame_tab.reshape(-1)

        def potential():
            hota.workspace.zero_()
            hip.hota_potential(overlaps, lout, rout, traj, geo.trk, 0, tab, geo.cells, geo.vecs, hota.workspace)

        def count():
            run.workspace.zero_()                                               # (pass 1 adds: every repeat starts from zero)
            hip.idf1_count(overlaps, lout, rout, traj, geo.trk, 0, tab, geo.cells, geo.vecs, run.workspace)

        zero = {'gpp_hota_potential': median_us(lambda: hota.workspace.zero_())[0], 'gpp_idf1_count': median_us(lambda: run.workspace.zero_())[0]}
        for what, launch in (('gpp_mot_assign', lambda: hip.mot_assign(overlaps, lab, counts, rows, ids, prm)), ('gpp_hota_potential', potential),
                             ('gpp_idf1_count', count), ('gpp_idf1_assign', run.finish)):
            med, low = median_us(launch)
            med, low = round(med - zero.get(what, 0.0), 2), round(low - zero.get(what, 0.0), 2)
            records.append({'what': 'launch', 'launch': what, 'workload': 'kitti', 'frames': N, 'D': D, 'A': A, 'sequences': len(packed.traj_ids),
                            'median_us': med, 'min_us': low,
                            'note': 'includes the copy of its host table and the allocation of its outputs; the median of zeroing the '
                                    'workspace ({} us) is subtracted'.format(zero.get(what, 0.0))})
        sides = geo.seq_tab[:, 1:3].tolist()
        records.append({'what': 'tables', 'workload': 'kitti', 'cells': geo.cells, 'counters': geo.vecs, 'workspace_bytes': int(run.workspace.numel()),
                        'largest_table': [int(v) for v in max(sides, key=lambda s: s[0] * s[1])]})
    with step_limit(600, 'kitti: evaluate_sequences'):
        M.evaluate_sequences(labels, tracks, device=True, idf1=True)            # (warm: the library, the allocator)
        t_with, t_without = [], []
        for _ in range(7):                                                      # (every leg ends in a download: the clock sees finished work)
            t0 = time.perf_counter()
            got = M.evaluate_sequences(labels, tracks, device=True, idf1=True)
            t_with.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            plain = M.evaluate_sequences(labels, tracks, device=True)
            t_without.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    host = I.add_idf1_np(plain, packed, params)          # (on the device form's codes, which tests hold equal to the NumPy form's)
    t_numpy = time.perf_counter() - t0
    same = [e['idf1'] for e in got['sequences']] == [e['idf1'] for e in host['sequences']] and got['all']['idf1'] == host['all']['idf1'] and \
        all(np.array_equal(a[k], b[k]) for a, b in zip(got['idf1_pairs'], host['idf1_pairs']) for k in a)
    t0 = time.perf_counter()
    ref = [definition_counts(p['C'], p['gc'], p['tc']) for p in got['idf1_pairs']]
    t_scipy = time.perf_counter() - t0
    mine = [(e['idf1']['integers']['idfn'], e['idf1']['integers']['idfp']) for e in got['sequences']]
    records.append({'what': 'whole', 'workload': 'kitti', 'frames': N, 'device_with_idf1_ms': round(statistics.median(t_with) * 1e3, 1),
                    'device_without_ms': round(statistics.median(t_without) * 1e3, 1), 'numpy_idf1_on_top_ms': round(t_numpy * 1e3, 1),
                    'equal': bool(same), 'scipy_definition_all_sequences_ms': round(t_scipy * 1e3, 2), 'definition_equal': bool(mine == ref),
                    'idf1': {k: got['all']['idf1'][k] for k in I.RATIOS}, 'integers': got['all']['idf1']['integers']})


def tables(records):
    out = ['| launch | workload | frames | D | A | median us | min us |', '|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'launch':
            out.append('| {launch} | {workload} | {frames} | {D} | {A} | {median_us} | {min_us} |'.format(**r))
    out += ['', '| tables | cells | counters | workspace bytes | largest table |', '|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'tables':
            out.append('| {workload} | {cells} | {counters} | {workspace_bytes} | {largest_table} |'.format(**r))
    out += ['', '| evaluate_sequences | frames | device with IDF1 ms | device without ms | NumPy IDF1 on top ms | equal | scipy (G+T)^2, all sequences ms | IDFN, IDFP equal |',
            '|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'whole':
            out.append('| {workload} | {frames} | {device_with_idf1_ms} | {device_without_ms} | {numpy_idf1_on_top_ms} | {equal} | '
                       '{scipy_definition_all_sequences_ms} | {definition_equal} |'.format(**r))
    out += ['', '| written tables | cells | gpp_idf1_assign median us | min us | steps of the longest table | us per step | scipy, rectangular ms | NumPy s | totals equal |',
            '|---|---|---|---|---|---|---|---|---|']
    for r in records:
        if r['what'] == 'table':
            out.append('| {tables} | {cells} | {gpp_idf1_assign_median_us} | {min_us} | {steps_longest_table} | {us_per_step} | {scipy_rectangular_ms} | '
                       '{numpy_s} | {totals_equal} |'.format(**r))
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'idf1'))
    ap.add_argument('--frames', type=int, default=8000)
    ap.add_argument('--steps-only', action='store_true')
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.steps_only:
        return count_steps(args.out)
    hip.require_device()
    steps_path = os.path.join(args.out, 'steps.json')
    steps = json.load(open(steps_path)) if os.path.isfile(steps_path) else {}
    records = []
    kitti(records, args.frames)
    tables_on_device(records, steps)
    with open(os.path.join(args.out, 'bench_idf1.jsonl'), 'w') as f:
        for r in records:
            f.write(json.dumps(r) + '\n')
    text = tables(records)
    with open(os.path.join(args.out, 'tables.md'), 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
