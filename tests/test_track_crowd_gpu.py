""" GPU tests of the tracker on crowded frames (csrc/track.hip: gpp_track_f64, gpp_track_optimal_f64, gpp_track_ego_f64): the kernel
against the NumPy form (utils/track.py) and the loop-written oracles on the scenes of tests/track_crowd_cases.py, whose reach -- rounds,
candidates, chunk fill, vertex counts -- and margins tests/test_track_crowd_cpu.py asserts.  The serial rule of DESIGN.md sections 4.28
and 4.32, as the oracle states it, is the truth: the kernel's rounds of mutually-best pairs, its 64-bit masks, its chunks of 4096 gated
pairs and its 128-lane clip must give the same ids, hits, state and rows.  Then the crowds in chunked calls, as one of several sequences
of a launch, in place, and behind ego records.

What each scene reaches:
    chain_n (2, 63, 64, 65, 128)   n rounds of ONE pair each: every round behind the first is a rescan against updated masks, and the
                                   loop runs to its bound min(slots, rows); rows scattered over all 128 indices, so the `hi` masks decide
                                   from n = 2 on; 63 / 64 / 65 step over the wavefront's edge on the slots' side; chain_128 is the
                                   longest dependency the rule allows
    lattice_64x64                  4096 gated pairs, all survivors: exactly one full chunk, s_pairs filled to its last word
    lattice_65x64                  4160 pairs: a second chunk of 64; slot 64 is the first of the upper wavefront
    lattice_100x90                 9000 pairs: two full chunks and a ragged one of 808; n is no multiple of anything
    lattice_128x128                16384 pairs: four full chunks; 8142 candidates with many equal keys taken in 5 rounds; frame 2 has
                                   pairs and no candidate (a stale table line would be one); frame 3 matches against moved slots
    lattice_128x128_back           the same with the rows shifted the other way: the tie rule (the smaller row) decides the matches, 8
                                   slots stay open and miss
    boundary_128, boundary_127     one survivor of the gate per slot, and the row order puts these decisive pairs on both sides of every
                                   chunk edge (pair 4095 | 4096, 8191 | 8192, 12287 | 12288), on the first pair and on the last: a pair
                                   dropped, doubled or read from the wrong chunk at an edge loses a track; with 127 rows the edges fall
                                   inside a slot's line
    turned_crowd                   128 x 128 rectangles at every angle: survivor lists of about 3000 per chunk, 8-vertex polygons, the
                                   clip's buffers used by all 128 lanes at once; the optimal form's matrix is full with > 1000 distinct
                                   cells; smoothed rows """
import numpy as np
import pytest
import torch

import test_track_gpu as G
import track_crowd_cases as C
import track_ego_oracle as E
import track_optimal_oracle as P
import track_oracle as O
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import track as T

pytestmark = pytest.mark.gpu

CASES = C.cases() + [(name + '_optimal', scene, opt) for name, scene, opt in C.optimal_cases()]
ASSIGNS = T.ASSIGNS


def option(metric, assign):
    opt = C.crowd_options(metric)
    return P.optimal(opt) if assign == 'optimal' else opt


@pytest.mark.parametrize('name,scene,opt', CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_host_form_and_the_oracle(name, scene, opt):
    """ ids, hits and every state field: ==; the rows bit for bit (alpha of smoothed rows within 4 float32 ulp).  r_y = 0 with dyadic
    numbers, or the margins tests/test_track_crowd_cpu.py asserts """
    frames = C.scenes()[scene]
    (o_rows, o_ids, o_hits, o_state), _, _ = C.oracle(scene, opt)
    n_rows, n_ids, n_hits, n_state = C.host(scene, opt)
    rows, ids, hits, state = T.track_rows_device(frames, opt)
    assert rows.dtype == np.float32 and ids.dtype == np.int32 and hits.dtype == np.int32 and rows.shape == frames.shape
    assert np.array_equal(ids, n_ids) and np.array_equal(ids, o_ids)
    assert np.array_equal(hits, n_hits) and np.array_equal(hits, o_hits)
    assert G.same_bytes(state, n_state) and O.same_state(o_state, state)
    assert G.rows_agree(rows, o_rows, opt['smooth']) and G.rows_agree(rows, n_rows, opt['smooth'])
    if not opt['smooth']:
        assert G.same_bytes(rows, frames)


def rows_equal(got, want, smooth):
    """ against the ego oracle, whose placement around the imported step may change a zero's sign (its docstring): ==, not bytes """
    cols = [c for c in range(36) if c != 25 or not smooth]
    return np.array_equal(got[..., cols], want[..., cols], equal_nan=True) and G.alpha_within_4_ulp(got[..., 25], want[..., 25])


@pytest.mark.parametrize('assign', ASSIGNS)
@pytest.mark.parametrize('metric,records', [('dist', 'TURNS'), ('bev', 'SHIFTS')])
def test_a_crowd_behind_ego_records(metric, records, assign):
    """ lattice_128x128 seen from a camera that moves by tests/track_ego_oracle.py's records -- quarter and half turns about Y with
    dyadic translations under 'dist', translations under 'bev' (behind a quarter turn a float32 r_y is no longer exact, and the
    lattice's equal overlaps are wanted equal) --: step 1b in all 128 slots, then the same crowded phases 3 and 4 """
    frames, ego = C.carried('lattice_128x128', getattr(E, records))
    opt = O.options(metric)
    opt = P.optimal(opt) if assign == 'optimal' else opt
    o_rows, o_ids, o_hits, o_state = E.track(frames, opt, ego)
    n_rows, n_ids, n_hits, n_state = T.track_rows_np(frames, opt, ego=ego)
    rows, ids, hits, state = T.track_rows_device(frames, opt, ego=ego)
    assert (n_hits[1] == 2).all() and (n_ids[2] == -1).all() and int(n_state['dropped']) == 128       # the crowd is found again behind the records
    assert np.array_equal(ids, n_ids) and np.array_equal(ids, o_ids)
    assert np.array_equal(hits, n_hits) and np.array_equal(hits, o_hits)
    assert G.same_bytes(state, n_state) and O.same_state(o_state, state)
    assert rows_equal(rows, o_rows, False) and G.rows_agree(rows, n_rows, False) and G.same_bytes(rows, frames)


@pytest.mark.parametrize('assign', ASSIGNS)
@pytest.mark.parametrize('metric', T.METRICS)
@pytest.mark.parametrize('scene', ['lattice_128x128', 'turned_crowd'])
def test_chunked_calls_give_the_same_bytes(scene, metric, assign):
    """ all frames in one call, in 1 + the rest, and in calls of one frame: the state a dense frame leaves is carried in full """
    frames = C.scenes()[scene]
    opt, N = option(metric, assign), len(frames)
    whole = G.device_chunks(frames, opt, [0, N])
    assert T.read_state(whole[3])['frames'] == N and (whole[2][-1] >= 2).sum() >= 100
    for cuts in ([0, 1, N], list(range(N + 1))):
        for got, want in zip(G.device_chunks(frames, opt, cuts), whole):
            assert G.same_bytes(got, want)


@pytest.mark.parametrize('assign', ASSIGNS)
@pytest.mark.parametrize('metric', T.METRICS)
def test_crowds_beside_a_sparse_sequence_equal_each_alone(metric, assign):
    """ one launch of S = 3 sequences -- the full lattice, the sparse drive, the turned crowd --: each equals the sequence alone.  The
    candidate table of a sequence index > 0 under full load; in the optimal form three workgroups with n = 128, <= 6 and 128 """
    frames = np.concatenate([C.scenes()['lattice_128x128'], C.drive_128()[:4], C.scenes()['turned_crowd']])
    seq = [0, 4, 8, 11]
    opt = option(metric, assign)
    rows, ids, hits, states = T.track_rows_device(frames, opt, seq_start=seq)
    assert states.shape == (3,) and states['frames'].tolist() == [4, 4, 3] and states['next_id'].tolist()[0::2] == [128, 128]
    assert 0 < int(states['next_id'][1]) <= 6
    for s, (a, b) in enumerate(zip(seq, seq[1:])):
        r, i, h, st = T.track_rows_device(frames[a:b], opt)
        assert G.same_bytes(rows[a:b], r) and G.same_bytes(ids[a:b], i) and G.same_bytes(hits[a:b], h) and G.same_bytes(states[s], st)


@pytest.mark.parametrize('assign', ASSIGNS)
@pytest.mark.parametrize('metric', T.METRICS)
def test_in_place(metric, assign):
    """ rows_out == rows_in and state_out == state_in on the full lattice: 128 rows are read before any is written """
    frames = C.scenes()['lattice_128x128']
    opt = option(metric, assign)
    want = T.track_rows_device(frames, opt)
    dev = hip.require_device()
    rows, state = torch.as_tensor(frames).to(dev), T.state_tensor(None, dev)
    out, ids, hits, state_out = T.track_rows_device(rows, opt, state, out=rows, state_out=state)
    assert out.data_ptr() == rows.data_ptr() and state_out.data_ptr() == state.data_ptr()
    assert G.same_bytes(rows.cpu().numpy(), want[0]) and G.same_bytes(ids.cpu().numpy(), want[1]) and G.same_bytes(hits.cpu().numpy(), want[2])
    assert G.same_bytes(T.read_state(state)[0], want[3]) and not G.same_bytes(want[0], frames)          # (smoothed: the rows were written)
