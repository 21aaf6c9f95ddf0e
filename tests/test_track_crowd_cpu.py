""" CPU tests of the tracker's crowded scenes (tests/track_crowd_cases.py): the NumPy form (utils/track.py) against the loop-written
oracles on every scene, metric and assignment, with the margins that let tests/test_track_crowd_gpu.py ask for equality; the
transcription of track.hip's phase 4 (rounds of mutually-best pairs, four 64-bit masks) against the serial rule on every frame; and the
reach assertions -- the rounds, the candidates, the chunk fill and the vertex counts that say the GPU file does drive the branches it
names.  Three deliberately wrong variants of the transcription must each be caught by the scenes. """
import numpy as np
import pytest

import test_track_optimal_cpu as OC
import track_crowd_cases as C
import track_oracle as O
from keras_retinanet_3D.utils import track as T

CASES = C.cases()
OPTIMAL = C.optimal_cases()
ids_of = lambda cases: [c[0] for c in cases]  # noqa: E731


def forms_agree(scene, opt):
    """ the cached host form against the cached oracle, as tests/test_track_cpu.same_as_oracle: ids, hits, every state field and the
    rows bit for bit (column 25 of smoothed rows within 4 float32 ulp) """
    (want_rows, want_ids, want_hits, want_state), values, matrices = C.oracle(scene, opt)
    got_rows, got_ids, got_hits, got_state = C.host(scene, opt)
    assert got_rows.dtype == np.float32 and got_ids.dtype == np.int32 and got_hits.dtype == np.int32
    assert np.array_equal(got_ids, want_ids) and np.array_equal(got_hits, want_hits)
    assert O.same_state(want_state, got_state)
    cols = [c for c in range(36) if c != 25 or not opt['smooth']]
    assert np.array_equal(got_rows[..., cols].view(np.uint32), want_rows[..., cols].view(np.uint32))
    close = np.abs(got_rows[..., 25].astype(np.float64) - want_rows[..., 25]) <= 4 * np.spacing(np.abs(want_rows[..., 25]))
    assert (close | (got_rows[..., 25].view(np.uint32) == want_rows[..., 25].view(np.uint32))).all()
    return values, matrices


def check_margins(scene, opt, values):
    """ no value within 1e-9 of the threshold; in the turned crowd no two candidates of a frame within 1e-9 of each other either (the
    chains and the lattices are exact: equal candidates are wanted there) """
    to_thr, apart = O.margins(values, opt)
    print(scene, opt['metric'], opt.get('assign', 'greedy'), 'to_thr', to_thr, 'apart', apart)
    assert to_thr > 1e-9, to_thr
    if scene == 'turned_crowd':
        assert apart > 1e-9, apart
    elif scene.startswith('lattice'):
        assert apart == 0.0


@pytest.mark.parametrize('name,scene,opt', CASES, ids=ids_of(CASES))
def test_host_form_equals_the_oracle(name, scene, opt):
    values, _ = forms_agree(scene, opt)
    check_margins(scene, opt, values)


def scaled_candidates(values, opt):
    """ o * 2^20, or q / thr^2 * 2^20, of every candidate: what section 4.32 takes the floor of """
    thr, dist = opt['threshold'], opt['metric'] == 'dist'
    cand = np.array([v for frame in values for v, _, _ in frame if ((v < thr * thr) if dist else (v > thr))])
    return (cand / (thr * thr) if dist else cand) * 1048576.0


@pytest.mark.parametrize('name,scene,opt', OPTIMAL, ids=ids_of(OPTIMAL))
def test_host_form_equals_the_oracle_under_the_optimal_assignment(name, scene, opt):
    """ ... and on every frame the oracle's matrix is cost_cells', both assignments reach scipy's total (tests/test_track_optimal_cpu.py's
    check).  In the turned crowd no candidate's scaled value lies within 1e-6 of an integer: a last bit of cos / sin moves it by 1e-10
    at the most, so the device's matrix is the host form's integer for integer, and one routine on one matrix gives one assignment;
    there n is 128 and more than 1000 cells are distinct """
    values, matrices = forms_agree(scene, opt)
    to_thr, _ = O.margins(values, opt)
    assert to_thr > 1e-9, to_thr
    host = OC.check_totals(C.scenes()[scene], opt, matrices)
    assert [len(h[3]) for h in host] == [len(m[3]) for m in matrices]
    if scene == 'turned_crowd':
        scaled = scaled_candidates(values, opt)
        off = np.abs(scaled - np.rint(scaled)).min()
        print(name, 'candidates', scaled.size, 'nearest to an integer', off)
        assert off > 1e-6, off
        for cost, ts, ds, pairs in host[1:]:
            assert cost.shape == (128, 128) and np.unique(cost[cost < T.SCALE]).size > 1000 and len(pairs) == 128


def frames_of(scene, opt):
    """ per frame (frame record, occupied slots, live rows) """
    return [(fr, np.flatnonzero(fr['occupied']), np.flatnonzero(fr['valid'])) for fr in C.trace(scene, opt)]


@pytest.mark.parametrize('name,scene,opt', CASES, ids=ids_of(CASES))
def test_the_rounds_of_phase_4_take_the_serial_rules_pairs(name, scene, opt):
    """ the transcription of track.hip's phase 4 == utils/track.greedy on every frame's candidate table, and what the scene reaches """
    report = []
    for f, (fr, ts, ds) in enumerate(frames_of(scene, opt)):
        matches, taken = C.phase4_rounds(fr['keys'], ts, ds)
        assert matches == sorted(T.greedy(fr['keys']))
        assert sorted(p for pairs in taken for p in pairs) == matches and all(taken)
        fill = C.chunk_fill(fr)
        report.append((f, int(np.isfinite(fr['keys']).sum()), [len(p) for p in taken], fill if opt['metric'] != 'dist' else None))
        n = min(ts.size, ds.size)
        if scene.startswith('chain') and f == 1:
            assert n == int(scene.split('_')[1]) and [len(p) for p in taken] == [1] * n          # as many rounds as the loop has
        if scene.startswith('lattice'):
            nT, nR = [int(v) for v in scene.split('_')[1].split('x')]
            if f in (1, 3):                              # the gate passes every pair of the lattice's cars: the chunks are full
                sizes = [min(C.CHUNK, ts.size * nR - a) for a in range(0, ts.size * nR, C.CHUNK)]
                assert ts.size == (nT if f == 1 else min(128, nT + nR)) and ds.size == nR and [s for s, _ in fill] == sizes
                assert sum(s for _, s in fill) >= nT * nR and fill[0] == (C.CHUNK, C.CHUNK)
            if f == 1:
                assert fill == [(s, s) for s in sizes] and len(matches) == (120 if scene.endswith('back') else n)
                assert len(taken) >= 4 and len(taken[0]) < n
            if f == 2:                                   # pairs are listed and none is a candidate: a stale table line would be one
                assert ts.size * ds.size >= nT * nR and not np.isfinite(fr['keys']).any() and matches == []
        if scene == 'turned_crowd' and f > 0:
            assert ts.size == ds.size == 128 and len(matches) == 128 and len(taken) >= 2
            if opt['metric'] != 'dist':                  # ragged survivor lists
                assert [s for s, _ in fill] == [C.CHUNK] * 4 and all(0 < s < C.CHUNK for _, s in fill)
    print(name, '(frame, candidates, pairs per round, (pairs, survivors) per chunk):', report)


def test_the_chunks_are_the_ones_the_issue_names():
    """ 4096 pairs: exactly one chunk; 4160: a second chunk of 64; 9000: a ragged last one; 16384: four """
    fills = {scene: C.chunk_fill(C.trace(scene, O.options('bev'))[1]) for scene in C.scenes() if scene.startswith('lattice')}
    assert fills == {'lattice_64x64': [(4096, 4096)], 'lattice_65x64': [(4096, 4096), (64, 64)],
                     'lattice_100x90': [(4096, 4096), (4096, 4096), (808, 808)], 'lattice_128x128': [(4096, 4096)] * 4,
                     'lattice_128x128_back': [(4096, 4096)] * 4}


@pytest.mark.parametrize('nR', C.BOUNDARY_SIZES)
def test_the_boundary_scenes_put_their_matches_on_the_chunk_edges(nR):
    """ one candidate per live row, each of them a match, and among them the pairs p = a * nR + c on both sides of every chunk edge, the
    first pair and the last: an off-by-one of phase 3 at an edge loses a track """
    scene, targets = 'boundary_{}'.format(nR), C.edge_targets(nR)
    assert targets[:3] == [0, 4095, 4096] and targets[-1] == 128 * nR - 1 and len(targets) == 8
    for metric in T.METRICS:
        opt, on_edges = O.options(metric), set()
        for fr, ts, ds in frames_of(scene, opt)[1:]:
            t, d = np.nonzero(np.isfinite(fr['keys']))
            assert ts.size == 128 and ds.size == nR and t.size == nR and np.unique(t).size == nR and np.unique(d).size == nR
            assert sorted(T.greedy(fr['keys'])) == sorted(zip(t.tolist(), d.tolist()))
            on_edges |= {int(np.searchsorted(ts, a)) * nR + int(np.searchsorted(ds, c)) for a, c in zip(t, d)} & set(targets)
            assert len(C.chunk_fill(fr)) == 4
        assert on_edges == set(targets)
        _, ids, hits, state = C.host(scene, opt)
        assert int(state['next_id']) == 128 and int((state['id1'] != 0).sum()) == 128 and (hits[-1] >= len(ids) - 2).sum() == nR


def test_late_pairs_straddle_64_in_both_directions():
    """ a pair taken after round 1 -- behind a rescan with updated masks -- with its slot in the upper wavefront and its row in the lower
    one, and another the other way round: in the long chain and in the full lattice, under every metric """
    for scene in ('chain_128', 'lattice_128x128'):
        for metric in T.METRICS:
            fr = C.trace(scene, O.options(metric))[1]
            late = [p for pairs in C.phase4_rounds(fr['keys'])[1][1:] for p in pairs]
            assert any(t >= 64 and d < 64 for t, d in late) and any(t < 64 and d >= 64 for t, d in late)
            assert any(t >= 64 and d >= 64 for t, d in late) and any(t < 64 and d < 64 for t, d in late)


def test_the_turned_crowd_clips_to_8_vertices():
    for metric in ('bev', '3d'):
        trace = C.trace('turned_crowd', C.crowd_options(metric))
        assert [C.most_vertices(fr) for fr in trace[1:]] == [8, 8]
    assert C.most_vertices(C.trace('lattice_128x128', O.options('bev'))[1]) == 4      # (r_y = 0: rectangles)


@pytest.mark.parametrize('fault', ['never_rescans', 'larger_row', 'no_hi_masks'])
def test_a_wrong_phase_4_is_caught(fault):
    """ the scenes discriminate: each deliberately wrong variant of the transcription differs from the serial rule on some frame """
    caught = []
    for name, scene, opt in CASES:
        for f, (fr, ts, ds) in enumerate(frames_of(scene, opt)):
            if ts.size and ds.size and C.phase4_rounds(fr['keys'], ts, ds, fault)[0] != sorted(T.greedy(fr['keys'])):
                caught.append((name, f))
    print(fault, 'caught by', caught)
    assert caught
    assert any(name.startswith('chain_128') or name.startswith('lattice_128x128') for name, _ in caught)


def test_the_transcription_on_small_tables():
    """ the tie rules and the defaults of phase4_rounds, by hand """
    inf = np.inf
    keys = np.full((128, 3), inf)
    assert C.phase4_rounds(keys) == ([], [])
    keys[5, 1], keys[5, 2], keys[70, 1] = 1.0, 1.0, 1.0                  # slot 5: rows 1 and 2 equal -> row 1; row 1: slots 5 and 70 equal -> slot 5
    assert C.phase4_rounds(keys) == ([(5, 1)], [[(5, 1)]])               # slot 70 has nothing left
    keys[70, 0] = 2.0
    assert C.phase4_rounds(keys) == ([(5, 1), (70, 0)], [[(5, 1)], [(70, 0)]])       # ... and finds row 0 behind a rescan
    assert C.phase4_rounds(keys, fault='never_rescans')[0] == [(5, 1)]
    assert C.phase4_rounds(keys, fault='larger_row')[0] == [(5, 2), (70, 1)]
    assert C.phase4_rounds(keys, slots=[5, 70, 100], rows=[0, 1, 2])[0] == sorted(T.greedy(keys))
