"""
The census of tests/decode_cases.py (no GPU): every constructed case shows, on the oracle (oracle/decode_np.py) and on the census's model
of nms_kernel's control flow, the branch of csrc/decode.hip it was built for -- the path (on chip, prefix, prefix then fallback,
fallback), where the histogram cut falls and where the cut thread's walk over its bins ends, the sorted ranks of the survivors and the
(slot, wavefront, lane) that holds each on chip, the line of the overlap test that decides a pair.  If a builder stops reaching its
branch, this file fails, not the GPU test silently.  Away from the threshold-boundary cases the oracle's NMS, which no golden pins, is
checked against a float64 overlap of the same float32 corners.
"""
import os
import re

import numpy as np
import pytest

import helpers
import decode_cases as dc
from oracle import decode_np


@pytest.mark.parametrize('name', dc.NAMES)
def test_case_reaches_its_branch(name):
    case = dc.get(name)
    cen = dc.census_of(name)
    assert dc.failed_claims(case, cen) == []
    assert case.claims and {c['list'] for c in case.claims} <= set(cen)
    (boxes, dims, scores, labels, orient), idx = case.oracle()
    counts = case.candidate_counts()
    for b in range(case.B):
        lists = [cen[(b, o)] for o in (range(4) if case.osf else (None,))]
        assert counts[b] == sum(c['K'] for c in lists)
        n = int((idx[b] >= 0).sum())
        assert n == min(case.max_det, sum(len(c['kept_ranks'][:case.max_det]) for c in lists))
        assert np.all(scores[b, n:] == -1) and np.all(scores[b, :n] > case.score_thr)          # a NaN score is never selected
        assert np.all(np.diff(scores[b, :n]) <= 0)
    for c in cen.values():                                   # the kept ranks ascend: the NMS walks the sorted list
        assert np.all(np.diff(c['kept_ranks']) > 0)
        assert all(0 <= q < dc.OWN and 0 <= w < dc.THREADS // dc.WAVE and 0 <= l < dc.WAVE for q, w, l in c['positions'])


def test_every_branch_has_a_case():
    """ every path, every slot 0..7 of the on-chip NMS, the first, a middle and the last wavefront and lane, every outcome of the cut
    thread's walk, every sort size of the table, both sides of the guard band and the division inside it, on chip and in global memory """
    paths, outcomes, slots, waves, lanes, sizes, branches = {}, {}, set(), set(), set(), set(), set()
    full_lists = 0
    for name in dc.NAMES:
        case = dc.get(name)
        cen = dc.census_of(name)
        for key, c in cen.items():
            paths.setdefault(c['path'], []).append(name)
            if c['outcome'] is not None:
                outcomes.setdefault(c['outcome'], []).append(name)
            if c['path'] == 'lds':
                sizes.add(c['K'])
            for q, w, l in c['positions']:
                slots.add(q), waves.add(w), lanes.add(l)
        for claim in case.claims:
            if 'pair_branch' in claim:
                branches.add((cen[claim['list']]['path'], claim['pair_branch'][1]))
        if case.osf and case.max_det == dc.MAX_DET_LIMIT:
            full_lists = max(full_lists, min(len(c['kept_ranks']) for c in cen.values()))
    assert set(paths) == set(dc.PATHS), sorted(set(dc.PATHS) - set(paths))
    assert set(outcomes) == set(dc.OUTCOMES), sorted(set(dc.OUTCOMES) - set(outcomes))
    assert slots == set(range(dc.OWN)) and {0, 7, 15} <= waves and {0, 63} <= lanes
    assert {k for k in dc.SORT_SIZES if k <= dc.LDS_KEYS} <= sizes and max(dc.SORT_SIZES) == dc.LDS_KEYS + 1
    for values in (None, 3):                                 # ... in both variants, and the size past the LDS in each
        name = 'sort_distinct' if values is None else 'sort_ties_b64'
        ks = [c['K'] for c in dc.census_of(name).values()]
        assert set(dc.SORT_SIZES) <= set(ks)
    assert dc.get('sort_ties_b64').B == dc.HEADER_SLOTS
    assert {('lds', 'division'), ('lds', 'sign_above'), ('lds', 'sign_below'), ('lds', 'no_area')} <= branches
    assert full_lists == dc.MAX_DET_LIMIT                    # four lists of 128: emit_osf_kernel's block of 512 is full
    # the on-chip path at eight pairs x five thresholds, the global path at three pairs x five
    assert len([n for n in dc.NAMES if n.startswith('pair_lds_')]) == 8 * 5 and len([n for n in dc.NAMES if n.startswith('pair_global_')]) == 3 * 5
    assert {dc.census_of(n)[(0, None)]['path'] for n in dc.NAMES if n.startswith('pair_global_')} == {'fallback', 'prefix+fallback'}
    assert [dc.census(c)[(0, None)]['path'] for c in dc.workspace_sequence()] == ['fallback', 'lds', 'lds', 'fallback']
    assert {dc.census_of(n)[(0, None)]['path'] for n in dc.STAGED.values()} == set(dc.PATHS)


@pytest.mark.parametrize('name', [n for n in dc.NAMES if n.startswith('pair_')])
def test_boundary_thresholds_straddle_the_oracle_decision(name):
    """ dc.iou_f32 is the quotient decode_np._iou_above compares: the oracle's answer turns exactly there, and the five thresholds of a
    pair sit on the sides their names say """
    case = dc.get(name)
    first, second = case.pair
    _, boxes = case.tables()
    a, b = boxes[0, first], boxes[0, second]
    q = dc.iou_f32(a, b)
    assert decode_np._iou_above(a, b, np.nextafter(q, dc.F(0))) and not decode_np._iou_above(a, b, q)
    which = name.split('_', 3)[3]
    assert case.iou_thr == dc.pair_threshold(q, which)
    assert decode_np._iou_above(a, b, case.iou_thr) == (which in ('below', 'band_below'))
    exact = float(dc.iou_exact(a, b[None])[0])
    # the float32 quotient against the exact ratio: three roundings in the intersection, four in the sum of the areas, the subtraction at most
    # doubles what it is handed (the union is at least half that sum) and rounds once, the division once: under 16 roundings of 2^-24 each
    assert abs(exact - float(q)) <= 16 * 2.0 ** -24 * exact
    if which.startswith('band'):
        assert 2.5e-6 < abs(float(case.iou_thr) / float(q) - 1) < 3.5e-6


@pytest.mark.parametrize('name', [n for n in dc.NAMES if not n.startswith(('pair_', 'identical_', 'no_nms'))])
def test_oracle_nms_against_an_exact_overlap(name):
    """ the oracle's greedy NMS (float32, one operation at a time) against the same loop on a float64 overlap of the same corners.  Every
    overlap of these cases is 0, 1 or further than 1e-3 from the threshold (asserted), so float32 rounding cannot turn a decision """
    case = dc.get(name)
    assert not case.boundary and case.kwargs.get('nms', True)
    folded, boxes = case.tables()
    for (b, o), c in dc.census_of(name).items():
        kept = dc.nms_exact(boxes[b], c['anchors'], case.max_det, float(case.iou_thr), margin=1e-3)
        assert kept == c['kept_anchors'][:case.max_det], (name, b, o)


def test_census_constants_are_the_kernels():
    src = open(os.path.join(helpers.ROOT, 'ground-plane-polling_amd', 'csrc', 'decode.hip')).read()
    for pattern in (r'constexpr int kNmsThreads = 1024;', r'constexpr int kLdsKeys = 8192;', r'constexpr int kHistBins = 4096;',
                    r'\(\(int\)\(key >> 32\) - 0x3D000000\) >> 14', r'constexpr int kOwn = kLdsKeys / kNmsThreads;',
                    r'own\[q\] = hist\[4 \* tid \+ q\]', r'if \(acc \+ own\[q\] <= kLdsKeys\)', r'if \(K <= kLdsKeys\)',
                    r'inter > tu \* 1\.000002f', r'inter < tu \* 0\.999998f', r'max_det > 128', r'if \(lists > 64\)'):
        assert re.search(pattern, src), 'csrc/decode.hip no longer reads `{}`: update the census in tests/decode_cases.py'.format(pattern)
    assert (dc.THREADS, dc.LDS_KEYS, dc.HIST_BINS, dc.OWN, dc.BINS_PER_THREAD) == (1024, 8192, 4096, 8, 4)
    one = np.array([1.0, 2.0 ** -5, 0.01], dc.F).view(np.uint32)
    assert dc.score_bin(one).tolist() == [2560, 0, 0]
    assert decode_np.sigmoid(dc.F(17.0)) == 1.0 and decode_np.sigmoid(dc.F(np.inf)) == 1.0 and decode_np.sigmoid(dc.F(-np.inf)) < 1e-37


def test_cases_stay_inside_the_gpu_budget():
    for name in dc.NAMES:
        case = dc.get(name)
        assert case.A <= 12288 and case.A % dc.NBA == 0 and case.B <= dc.HEADER_SLOTS, name
        assert case.A <= dc.LDS_KEYS + 24 or any(c['K'] > dc.LDS_KEYS for c in dc.census_of(name).values()), name    # large only where needed
