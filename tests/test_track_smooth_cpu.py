""" CPU tests of the offline smoother: the NumPy form (utils/track_smooth.py) against the loop-written oracle
(tests/track_smooth_oracle.py) on every output word; the forward pass against the tracker's own Kalman filter; the smoothed means and
position covariances against a batch weighted least-squares solve of the whole trajectory; exact cases; the direction of the error on a
seeded scene; the segmenting; the fills; the C ABI's refusals (host code: they come before any launch); the command lines. """
import ctypes
import math
import os

import numpy as np
import pytest

import track_ego_oracle as E
import track_kf_oracle as K
import track_smooth_cases as C
import track_smooth_oracle as R
from track_smooth_cases import KALMAN, same_outputs, write_run
from track_oracle import padding, row
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import track as T
from keras_retinanet_3D.utils import track_smooth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = C.NOISE


def as_oracle(index):
    return [(int(index.seg_id[s]), int(index.seg_frame[s]), index.cell_row[index.seg_start[s]:index.seg_start[s + 1]].tolist())
            for s in range(len(index.seg_frame))]


def against_oracle(rows, ids, seq_start, G, noise=NOISE, ego=None):
    index = S.segments_of(ids, seq_start, G, rows)
    assert as_oracle(index) == R.segments(ids, seq_start, G, rows)
    got = S.smooth_np(rows, index, noise, ego)
    same_outputs(got, R.smooth(rows, as_oracle(index), noise, ego))
    return index, got


# ---------------------------------------------------------------------------------------------------- NumPy form == oracle
@pytest.mark.parametrize('kind', [None, 'identity', 'turns', 'yaw', 'general'])
@pytest.mark.parametrize('G', [0, 1, 3])
def test_numpy_form_equals_the_oracle(kind, G):
    rows, ids = C.scene(7 + G, N=24, D=6, cars=5, seq_start=[0, 10, 24])
    index, got = against_oracle(rows, ids, [0, 10, 24], G, ego=C.records(kind, 24))
    length = np.diff(index.seg_start)
    assert (length == 1).any() and (length >= 3).any() and (got[2].shape[0] > 0 or G == 0)
    assert (got[1] != 0).any() and not np.array_equal(got[0], rows)


def test_a_restart_is_the_same_in_both_forms():
    """ det not > 0: a radial noise so steep that one far row's R overflows -- the cell restarts as at a birth, the step into it is skipped """
    noise = dict(NOISE, radial=(0.1, 1e150))
    rows = np.stack([padding(1) for _ in range(5)])
    for f, (x, z) in enumerate([(1e-3, 2e-3), (2e-3, 3e-3), (0.0, 1e6), (3e-3, 1e-3), (2e-3, 2e-3)]):
        rows[f, 0] = row(0.9, x, z)
    ids = np.zeros((5, 1), np.int32)
    keep = {}
    index = S.segments_of(ids, None, 0, rows)
    got = S.smooth_np(rows, index, noise, keep=keep)
    same_outputs(got, R.smooth(rows, as_oracle(index), noise))
    assert np.isnan(keep['filtered'][4:, 2]).any()                       # the restarted cell carries the overflowed R
    assert np.array_equal(keep['smoothed'][:, 1], keep['filtered'][:, 1])   # the step into it was skipped


# ---------------------------------------------------------------------------------------------------- the forward pass is the tracker's
@pytest.mark.parametrize('with_records', [False, True])
def test_the_forward_pass_is_the_trackers(with_records):
    """ one car through track_rows_np with 'filter': 'kalman', 12 frames, two of them missed: the filtered state of the segment's last cell
    is the slot's state and covariance, word for word.  The records turn about Y only, so the y term the smoother leaves out is a zero """
    rows = np.stack([padding(1) for _ in range(12)])
    for f in range(12):
        if f not in (4, 9):
            rows[f, 0] = row(0.9, 1.0 + 0.3 * f + 0.1 * (f % 3), 20.0 + 0.7 * f - 0.2 * (f % 2))
    ego = C.records('yaw', 12) if with_records else None
    opt = K.options('dist', 8.0)
    _, ids, _, state, cov = T.track_rows_np(rows, opt, ego=ego)
    assert int(state['next_id']) == 1 and (ids[:, 0] >= 0).sum() == 10
    index = S.segments_of(ids, None, 2, rows)
    assert len(index.seg_frame) == 1 and index.cell_row.size == 12
    keep = {}
    S.smooth_np(rows, index, opt['noise'], ego, keep=keep)
    last = keep['filtered'][:, 11]
    slot = int(np.flatnonzero(state['id1'])[0])
    assert [last[0], last[1], last[2], last[3]] == [state['box'][k][slot] for k in (0, 2, 7, 9)]
    assert np.array_equal(last[4:], cov[:, slot])


def test_the_forward_pass_is_the_trackers_on_a_frame_of_cars():
    """ the same comparison between the two callers of utils/track_kf.py on a frame of four cars, 10 frames under the 'general' records
    (yaw and pitch in frame 1), car 1 missed in frame 4 and car 2 in frame 6: of every identity the filtered words of the segment's last
    cell are the slot's state and covariance, all 14, ==.  The rows stand where the records carry the cars, plus a small step of their
    own.  What makes the two forms one filter here, and is written into the scene:
      - y = 0 in every row and gain b = 0, so y and vy stay 0 and the pitch's y terms, which the smoother leaves out, are zeros;
      - the noise is so steep (sigma 1e75 rho) that for the far car, at 200 m, det S overflows to inf - inf in EVERY matched step, while
        the three cars within 12 m stay finite: the tracker takes its fallback there and the smoother restarts.  With gain a = 1 the
        fallback's mean is pred + (row - pred) = the row exactly (the two lie within a factor of two: the difference is exact), its
        velocity has been 0 since birth, and both set P as at a birth from the row: the restart's words;
      - the birth speed (1e76) is on the noise's scale, so the near cars' velocity gains are of order 1: they end at velocities near
        their steps, with B and C blocks that every update has moved """
    N, steps = 10, [(0.125, 0.25), (-0.0625, 0.5), (0.25, -0.125), (0.5, 0.5)]
    ego = C.records('general', N)
    where = [(-3.0, 9.0), (2.0, 6.0), (5.0, 10.0), (141.0, 141.0)]           # three near cars, one far: the car of row k
    missed = {(1, 4), (2, 6)}
    rows = np.stack([padding(4) for _ in range(N)])
    for f in range(N):
        e = ego[f]
        if f:
            where = [(e[0] * x + e[2] * z + e[9] + sx, e[6] * x + e[8] * z + e[11] + sz) for (x, z), (sx, sz) in zip(where, steps)]
        for k, (x, z) in enumerate(where):
            if (k, f) not in missed:
                rows[f, k] = row(0.9 - 0.1 * k, x, z, y=0.0)
    noise = dict(NOISE, radial=(0.1, 1e75), tangential=(0.1, 0.5e75), birth_speed=1e76)
    opt = K.options('dist', 8.0, noise=noise, gains=(1.0, 0.0, 0.25))
    _, ids, _, state, cov = T.track_rows_np(rows, opt, ego=ego)
    assert int(state['next_id']) == 4 and int(state['dropped']) == 0 and (ids >= 0).sum() == 4 * N - 2
    index = S.segments_of(ids, None, 2, rows)
    assert index.seg_id.tolist() == [0, 1, 2, 3] and np.diff(index.seg_start).tolist() == [N] * 4 and (index.cell_row < 0).sum() == 2
    keep = {}
    S.smooth_np(rows, index, noise, ego, keep=keep)
    for s, who in enumerate(index.seg_id):
        last = keep['filtered'][:, index.seg_start[s + 1] - 1]
        slot = int(np.flatnonzero(state['id1'] == who + 1)[0])
        assert np.isfinite(last).all()
        assert [last[0], last[1], last[2], last[3]] == [state['box'][k][slot] for k in (0, 2, 7, 9)]
        assert np.array_equal(last[4:], cov[:, slot])
        born = last[2:4].tolist() == [0.0, 0.0] and last[7:].tolist() == [0.0, 0.0, 0.0, 0.0, 1e152, 0.0, 1e152]
        assert born == (who == 3)                                            # the far car restarted, the near ones were updated


# ---------------------------------------------------------------------------------------------------- an independent check
def least_squares(rows, index, noise, ego):
    """ one segment as a batch weighted least-squares problem over all its states: the birth prior, one process residual per step, one
    measurement residual per detected cell -> (means (cells, 4), covariances (cells, 4, 4)) by np.linalg """
    cells = index.cell_row
    n, flat = cells.size, rows.reshape(-1, 36).astype(np.float64)
    frame = int(index.seg_frame[0])
    blocks, rhs = [], []

    def whiten(cov, lines, b):
        L = np.linalg.cholesky(cov)
        blocks.append(np.linalg.solve(L, lines))
        rhs.append(np.linalg.solve(L, b))

    def noise_of(r):
        rxx, rxz, rzz = T.row_noise(rows.reshape(-1, 36)[r:r + 1], noise)[:, 0]
        return np.array([[rxx, rxz], [rxz, rzz]])

    first = np.zeros((4, 4 * n))
    first[:, :4] = np.eye(4)
    prior = np.zeros((4, 4))
    prior[:2, :2], prior[2:, 2:] = noise_of(cells[0]), np.eye(2) * noise['birth_speed'] ** 2
    whiten(prior, first, np.array([flat[cells[0], 19], flat[cells[0], 21], 0.0, 0.0]))
    Q = np.diag([noise['process'][0]] * 2 + [noise['process'][1]] * 2)
    F = np.array([[1.0, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]])
    for c in range(1, n):
        G, u = np.eye(4), np.zeros(4)
        if ego is not None:
            e = ego[frame + c]
            G = np.kron(np.eye(2), np.array([[e[0], e[2]], [e[6], e[8]]]))
            u[:2] = e[9], e[11]
        lines = np.zeros((4, 4 * n))
        lines[:, 4 * c:4 * c + 4], lines[:, 4 * c - 4:4 * c] = np.eye(4), -G.dot(F)
        whiten(G.dot(Q).dot(G.T), lines, u)
        if cells[c] >= 0:
            lines = np.zeros((2, 4 * n))
            lines[0, 4 * c], lines[1, 4 * c + 1] = 1.0, 1.0
            whiten(noise_of(cells[c]), lines, np.array([flat[cells[c], 19], flat[cells[c], 21]]))
    A, b = np.concatenate(blocks), np.concatenate(rhs)
    mean = np.linalg.lstsq(A, b, rcond=None)[0]
    cov = np.linalg.inv(A.T.dot(A))
    return mean.reshape(n, 4), np.stack([cov[4 * c:4 * c + 4, 4 * c:4 * c + 4] for c in range(n)])


# the largest deviation of a smoothed mean (metres) or position covariance word (square metres) from the batch solve over the eight
# cases below, measured on the CPU: 2.2e-13 (means) and 7.6e-13 (covariances); the bar is 100 x the larger, and never looser than 1e-9
MEASURED_DEVIATION = 7.6e-13
BAR = min(100 * MEASURED_DEVIATION, 1e-9)


@pytest.mark.parametrize('with_records', [False, True])
@pytest.mark.parametrize('cells', [2, 3, 12, 40])
def test_smoothed_means_and_covariances_solve_the_batch_problem(cells, with_records):
    rows, ids, _ = C.receding(100 + cells, frames=cells, miss=0.25)
    ego = C.records('yaw', cells) if with_records else None
    index = S.segments_of(ids, None, cells, rows)
    assert len(index.seg_frame) == 1 and index.cell_row.size == cells
    keep = {}
    S.smooth_np(rows, index, NOISE, ego, keep=keep)
    mean, cov = least_squares(rows, index, NOISE, ego)
    sm = keep['smoothed']
    dev_mean = np.abs(sm[0:2].T - mean[:, 0:2]).max()
    dev_cov = max(np.abs(sm[4] - cov[:, 0, 0]).max(), np.abs(sm[5] - cov[:, 0, 1]).max(), np.abs(sm[6] - cov[:, 1, 1]).max())
    print('cells {} records {}: mean {:.3g} m, covariance {:.3g} m^2'.format(cells, with_records, dev_mean, dev_cov))
    assert dev_mean <= BAR and dev_cov <= BAR


# ---------------------------------------------------------------------------------------------------- exact cases
def test_a_segment_of_one_cell_is_a_bit_copy():
    rows, ids = C.chains(3, 1)
    index, got = against_oracle(rows, ids, None, 2)
    assert np.diff(index.seg_start).tolist() == [1, 1, 1]
    assert got[0].tobytes() == rows.tobytes() and not got[1].any() and got[2].shape == (0, 36) and got[3].shape == (0, 3)


def test_a_quarter_turn_swaps_the_words_bit_for_bit():
    """ section 4.34's pin: under a quarter turn about Y 0 * a is a zero and a + 0 is a, so the predicted x and z words change places """
    rows, ids = C.chains(1, 3)
    index = S.segments_of(ids, None, 0, rows)
    plain, turned = {}, {}
    S.smooth_np(rows, index, NOISE, None, keep=plain)
    left = np.array([E.IDENTITY, E.record(E.LEFT, [0.5, 0.125, -0.25], E.QUARTER), E.IDENTITY])
    S.smooth_np(rows, index, NOISE, left, keep=turned)
    p, t = plain['predicted'][:, 1], turned['predicted'][:, 1]
    assert t[0] == p[1] + 0.5 and t[1] == -p[0] - 0.25 and t[2] == p[3] and t[3] == -p[2]
    assert t[4] == p[6] and t[6] == p[4] and t[5] == -p[5]               # Axx <-> Azz
    assert t[7] == p[10] and t[10] == p[7] and t[11] == p[13] and t[13] == p[11]


# ---------------------------------------------------------------------------------------------------- direction only
def test_smoothing_lowers_the_error_and_fills_beat_the_prediction():
    """ one car receding from 15 m under the noise model itself, 40 frames, a fifth missed: RMS position error raw > filtered > smoothed at
    the detected frames, and forward prediction > fill at the missed ones.  Only the order is asserted """
    rows, ids, truth = C.receding(3)
    index = S.segments_of(ids, None, 6, rows)
    assert len(index.seg_frame) == 1
    keep = {}
    out, _, fills, _ = S.smooth_np(rows, index, NOISE, keep=keep)
    seen, gap = index.cell_row >= 0, index.cell_row < 0
    assert gap.sum() >= 4 and fills.shape[0] == gap.sum()
    rms = lambda xz, where: math.sqrt(((xz[where] - truth[where]) ** 2).sum(axis=1).mean())  # noqa: E731
    raw = rms(rows[:, 0][:, [19, 21]].astype(np.float64), seen)
    filtered, smoothed = rms(keep['filtered'][0:2].T, seen), rms(keep['smoothed'][0:2].T, seen)
    assert raw > filtered > smoothed
    assert rms(keep['predicted'][0:2].T, gap) > rms(keep['smoothed'][0:2].T, gap)
    assert np.array_equal(fills[:, [19, 21]], keep['smoothed'][0:2].T[gap].astype(np.float32))
    assert np.array_equal(out[seen, 0][:, [19, 21]], keep['smoothed'][0:2].T[seen].astype(np.float32))


# ---------------------------------------------------------------------------------------------------- segmenting
def test_a_gap_of_exactly_max_gap_is_filled_and_one_more_splits():
    for G in (0, 1, 3):
        rows, ids = C.chains(2, 3, step=G + 1)                           # G gaps between two detections
        index, got = against_oracle(rows, ids, None, G)
        assert np.diff(index.seg_start).tolist() == [2 * G + 3] * 2 and got[2].shape[0] == 4 * G
        if G:
            split = S.segments_of(ids, None, G - 1, rows)
            assert np.diff(split.seg_start).tolist() == [1] * 6 and split.seg_id.tolist() == [0, 0, 0, 1, 1, 1]
            assert split.seg_frame.tolist() == [0, G + 1, 2 * G + 2] * 2


def test_rows_without_an_identity_or_a_position_are_untouched_and_sequences_stay_apart():
    rows, ids = C.chains(2, 6)
    ids[:, 1] = -1                                                       # the second car has no identity
    rows[2, 0, 19:26] = np.nan                                           # a row of the first without a position: a gap
    seq = [0, 3, 6]                                                      # the same id in two sequences: two segments
    index, got = against_oracle(rows, ids, seq, 1)
    assert index.seg_frame.tolist() == [0, 3] and np.diff(index.seg_start).tolist() == [2, 3] and index.seg_id.tolist() == [0, 0]
    assert got[0][:, 1].tobytes() == rows[:, 1].tobytes() and got[0][2, 0].tobytes() == rows[2, 0].tobytes() and got[2].shape[0] == 0
    assert not got[1][:, 1].any() and not got[1][2, 0].any() and got[1][0, 0].all()
    one = S.segments_of(ids, None, 1, rows)                              # as one sequence: frames 0 1 . 3 4 5 with one gap
    assert np.diff(one.seg_start).tolist() == [6] and one.cell_row.tolist() == [0, 2, -1, 6, 8, 10]
    outside = S.segments_of(ids, [1, 3], 1, rows)                        # frames outside every sequence have no cell
    assert outside.cell_row.tolist() == [2]
    nobody = S.segments_of(np.full_like(ids, -1), None, 1, rows)         # no identity at all: no segment, and nothing changes
    assert nobody.seg_start.tolist() == [0] and nobody.cell_row.size == 0 and nobody.seg_frame.size == 0
    assert S.smooth_np(rows, nobody, NOISE)[0].tobytes() == rows.tobytes()
    for shape in ((0, 4, 36), (3, 0, 36)):
        empty = S.smooth_np(np.zeros(shape, np.float32), S.segments_of(np.zeros(shape[:2], np.int32), None, 1), NOISE)
        assert empty[0].shape == shape and empty[1].shape == shape[:2] + (3,) and empty[2].shape == (0, 36) and empty[3].shape == (0, 3)


def test_an_id_twice_in_a_frame_raises():
    rows, ids = C.chains(2, 3)
    ids[1, 1] = 0
    with pytest.raises(ValueError, match='twice in frame 1'):
        S.segments_of(ids, None, 1, rows)
    with pytest.raises(ValueError, match='twice'):
        R.segments(ids, None, 1, rows)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='max_gap'):
            S.segments_of(ids, None, bad)


def test_the_order_of_the_segments_changes_no_output():
    rows, ids = C.scene(5, N=16, D=4, cars=4, miss=0.4)
    index = S.segments_of(ids, None, 3, rows)
    want = S.smooth_np(rows, index, NOISE)
    back = S.reorder(index, np.arange(len(index.seg_frame))[::-1])
    got = S.smooth_np(rows, back, NOISE)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
    # the fills follow the cells: the same rows, in the other order
    key = lambda f: sorted(map(bytes, f))  # noqa: E731
    assert key(got[2]) == key(want[2]) and got[2].shape[0] > 1


# ---------------------------------------------------------------------------------------------------- fills
def test_fills_take_the_short_way_round_and_codes_from_the_earlier_neighbour():
    rows = np.stack([padding(1) for _ in range(4)])
    rows[0, 0] = row(0.9, 1.0, 20.0, ry=3.0, orient=2)
    rows[3, 0] = row(0.3, 2.5, 23.0, ry=-3.0, orient=1, h=1.8, y=1.5)
    rows[0, 0, 33:36], rows[3, 0, 33:36] = (7.0, 8.0, 9.0), (1.0, 2.0, 3.0)
    ids = np.array([[0], [-1], [-1], [0]], np.int32)
    index, got = against_oracle(rows, ids, None, 2)
    fills = got[2]
    assert fills.shape == (2, 36)
    delta = 2.0 * math.pi - 6.0                                          # from 3.0 on across +-pi to -3.0
    assert abs(float(fills[0, 32]) - (3.0 + delta / 3.0)) < 1e-6 and abs(float(fills[1, 32]) - (3.0 + 2.0 * delta / 3.0 - 2.0 * math.pi)) < 1e-6
    assert (fills[:, 14] == 2).all() and (fills[:, 13] == 0).all() and np.array_equal(fills[:, 33:36], np.array([[7.0, 8.0, 9.0]] * 2, np.float32))
    assert np.array_equal(fills[:, 12], (0.9 + np.array([1.0, 2.0]) / 3.0 * (np.float64(np.float32(0.3)) - np.float64(np.float32(0.9)))).astype(np.float32))
    assert np.allclose(fills[:, 16], [1.6, 1.7]) and np.allclose(fills[:, 31], [1.6, 1.55]) and np.allclose(fills[:, 20], [1.6, 1.55])
    # a detection facing the other way is read as facing the track's way: the half-turn rule of section 4.28
    rows[3, 0, 32] = np.float32(3.0 - math.pi + 0.3)
    _, got = against_oracle(rows, ids, None, 2)
    assert abs(float(got[2][0, 32]) - 3.1) < 1e-6
    # alpha follows the fill's own r_y and smoothed position
    want = T.wrap(got[2][:, 32].astype(np.float64) - np.arctan2(got[2][:, 19].astype(np.float64), got[2][:, 21].astype(np.float64)))
    assert np.abs(got[2][:, 25] - want).max() < 1e-5
    # merge_fills: the fills behind the rows of their frames, with the segment's id and the hits of the detection before
    merged = S.merge_fills(got[0], ids, np.array([[1], [0], [0], [2]], np.int32), index, got[2])
    assert [len(r) for r in merged[0]] == [1, 2, 2, 1] and merged[1][1].tolist() == [-1, 0] and merged[2][2].tolist() == [0, 1]
    assert merged[0][2][1].tobytes() == got[2][1].tobytes()
    assert T.tracking_lines(1, merged[0][1], merged[1][1], merged[2][1]).startswith('1 0 Car -1 -1 ')


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_makefile_and_binding():
    text = open(os.path.join(ROOT, 'include', 'gpp.h')).read()
    assert 'int gpp_track_smooth_workspace_bytes(int N, int n_seg, long long cells, size_t* bytes);' in text
    assert 'const gpp_track_kf_params* kf' in text[text.index('int gpp_track_smooth_f64('):]
    makefile = open(os.path.join(ROOT, 'ground-plane-polling_amd', 'csrc', 'Makefile')).read()
    assert 'track_smooth.hip' in makefile[makefile.index('SRCS_EXACT ='):].splitlines()[0]
    assert '$(OBJ)/track_smooth.o: track_smooth.hip' in makefile
    assert tuple(S.CODE_COLS) == (13, 14, 33, 34, 35)
    n = ctypes.c_size_t(0)
    lib = hip.lib()
    assert lib.gpp_track_smooth_workspace_bytes(10, 3, 20, ctypes.byref(n)) == 0 and n.value == hip.track_smooth_workspace_bytes(10, 3, 20)
    assert n.value >= 28 * 8 * (20 + 64 * 10) + 5 * 8 * 20 + 10 * 128 and n.value % 8 == 0
    assert lib.gpp_track_smooth_workspace_bytes(10, 3, 20, None) == -1
    for bad in ((-1, 3, 20), (10, -1, 20), (10, 3, -1)):
        assert lib.gpp_track_smooth_workspace_bytes(*(bad + (ctypes.byref(n),))) == -1


FAKE = 4096     # a device pointer no host code looks at: every refusal, and the workspace check behind them all, returns before any HIP call


def smooth_call(N=4, D=2, seg_start=(0, 3), seg_frame=(1,), cell_row=(2, -1, 6), kf=None, ego=None, null=(), rows_in=FAKE, rows_out=FAKE,
                row_cov=0, fill_rows=FAKE, fill_cov=0, workspace=FAKE):
    """ with a workspace of 0 bytes a call that passes every argument check is GPP_ERR_WORKSPACE (-2): -1 then means the argument """
    k = hip.TrackKfParams(**dict(K_GOOD, **(kf or {})))
    ss = np.array(seg_start, np.int64)
    sf, cr = np.array(seg_frame, np.int32), np.array(cell_row, np.int32)
    e = None if ego is None else np.ascontiguousarray(ego, np.float64)
    arg = lambda name, value: None if name in null else value  # noqa: E731
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return hip.lib().gpp_track_smooth_f64(arg('rows_in', p(rows_in)), N, D, arg('seg_start', ss.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
                                          arg('seg_frame', sf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                                          arg('cell_row', cr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), len(sf),
                                          arg('kf', ctypes.byref(k)), None if e is None else e.ctypes.data_as(ctypes.c_void_p),
                                          arg('rows_out', p(rows_out)), p(row_cov), arg('fill_rows', p(fill_rows)), p(fill_cov),
                                          arg('workspace', p(workspace)), 0, None)


K_GOOD = dict(radial0=0.1, radial1=0.05, tangential0=0.1, tangential1=0.005, q_pos=0.01, q_vel=0.01, birth_speed=2.0, reserved=0)


def test_c_abi_refuses_before_any_launch():
    nan, inf = float('nan'), float('inf')
    records = np.array([E.IDENTITY] * 4)
    assert smooth_call() == -2 and smooth_call(ego=records) == -2 and smooth_call(rows_out=FAKE + 36 * 8 * 4) == -2
    assert smooth_call(row_cov=FAKE, fill_cov=FAKE) == -2 and smooth_call(D=128, cell_row=(128, -1, 3 * 128 + 127)) == -2
    # null required pointers
    for name in ('rows_in', 'rows_out', 'seg_start', 'seg_frame', 'cell_row', 'kf', 'fill_rows', 'workspace'):
        assert smooth_call(null=(name,)) == -1, name
    assert smooth_call(cell_row=(2, 4, 6), null=('fill_rows',)) == -2    # (no gap: no fill rows are needed)
    # sizes
    assert smooth_call(D=129) == -1 and smooth_call(N=-1) == -1 and smooth_call(D=-1) == -1
    assert smooth_call(N=1 << 24, D=128) == -1                           # N * D beyond 2^31 - 1
    assert smooth_call(N=0) == -1 and smooth_call(D=0) == -1             # cells without rows
    # the noise refusals of gpp_track_kf_f64
    for name in ('radial0', 'tangential0', 'birth_speed'):
        for value in (0.0, -0.5, nan, inf, -inf):
            assert smooth_call(kf={name: value}) == -1, (name, value)
    for name in ('radial1', 'tangential1', 'q_pos', 'q_vel'):
        assert smooth_call(kf={name: 0.0}) == -2
        for value in (-1e-300, nan, inf, -inf):
            assert smooth_call(kf={name: value}) == -1, (name, value)
    for word in (1, -1, 1 << 40):
        assert smooth_call(kf={'reserved': word}) == -1
    # offsets that do not ascend
    for seg_start, seg_frame in (((1, 3), (1,)), ((0, 0), (1,)), ((0, 2, 2), (1, 1)), ((0, 2, 1), (1, 1)), ((0, -1), (1,))):
        assert smooth_call(seg_start=seg_start, seg_frame=seg_frame) == -1, seg_start
    # a frame or a row index out of range, a row outside its cell's frame or in two cells
    assert smooth_call(seg_frame=(-1,)) == -1 and smooth_call(seg_frame=(2,)) == -1 and smooth_call(seg_frame=(0,)) == -1
    for cell_row in ((2, -1, 8), (2, -2, 6), (2, -1, 4), (0, -1, 6), (2, 3, 6)):
        assert smooth_call(cell_row=cell_row) == -1, cell_row
    assert smooth_call(seg_start=(0, 1, 2), seg_frame=(1, 1), cell_row=(2, 2)) == -1
    assert smooth_call(seg_start=(0, 1, 2), seg_frame=(1, 1), cell_row=(2, 3)) == -2
    # a segment whose first or last cell is a gap
    assert smooth_call(cell_row=(-1, 4, 6)) == -1 and smooth_call(cell_row=(2, 4, -1)) == -1
    # the records: a value that is not finite, a padding word that is not 0 -- in any frame
    for f, k, value in ((0, 0, nan), (3, 12, inf), (2, 9, -inf), (1, 13, 1.0), (3, 15, nan)):
        bad = records.copy()
        bad[f, k] = value
        assert smooth_call(ego=bad) == -1, (f, k)
    # alignment
    assert smooth_call(rows_in=FAKE + 2) == -3 and smooth_call(fill_rows=FAKE + 1) == -3 and smooth_call(workspace=FAKE + 4) == -3
    assert smooth_call(row_cov=FAKE + 4) == -3 and smooth_call(fill_cov=FAKE + 4) == -3
    # nothing to do is no error: no segment at all, with and without rows
    assert smooth_call(N=0, D=0, seg_start=(0,), seg_frame=(), cell_row=(), null=('rows_in', 'rows_out', 'fill_rows', 'workspace', 'seg_frame', 'cell_row')) == 0
    # the host side refuses the same index before the library sees it
    rows = np.zeros((4, 2, 36), np.float32)
    for bad in (S.Index(np.array([0, 3]), np.array([1]), np.array([2, -1, 4]), np.array([0]), 1),
                S.Index(np.array([0, 3]), np.array([2]), np.array([2, -1, 6]), np.array([0]), 1),
                S.Index(np.array([0, 3]), np.array([1]), np.array([-1, 4, 6]), np.array([0]), 1),
                S.Index(np.array([0, 1, 2]), np.array([1, 1]), np.array([2, 2]), np.array([0, 1]), 1)):
        with pytest.raises(ValueError):
            S.smooth_np(rows, bad, NOISE)


# ---------------------------------------------------------------------------------------------------- the command lines
def test_track_results_rts_writes_the_smoothed_filled_file_and_lowers_fn(tmp_path, capsys):
    from keras_retinanet_3D.bin import track_results
    common = write_run(tmp_path)
    plain = track_results.main(common + ['--labels', str(tmp_path / 'l.txt')])
    before = (tmp_path / 'tracks.txt').read_text()
    smooth = track_results.main(common + ['--labels', str(tmp_path / 'l.txt'), '--rts'] + KALMAN)
    after = (tmp_path / 'tracks.txt').read_text()
    assert plain['all']['fn'] == 2 and smooth['all']['fn'] == 0 and smooth['all']['tp'] == 8 and smooth['all']['frag'] < plain['all']['frag'] + 1
    assert len(before.splitlines()) == 6 and [int(line.split()[0]) for line in after.splitlines()] == list(range(8))
    assert {line.split()[1] for line in after.splitlines()} == {'0'} and '2 fills' in capsys.readouterr().out
    # the file is tracking_lines over merge_fills over smooth_np over the raw rows of the same run
    names, frames = track_results.read_sequence(str(tmp_path / 'kitti'))
    _, ids, hits, _ = T.track_rows_np(frames, ('dist', 3.0))
    noise = {'radial': (0.1, 0.05), 'tangential': (0.1, 0.005), 'process': (0.01, 0.01), 'birth_speed': 2.0}
    rows, mids, mhits, fills = S.smooth_tracks(frames, ids, hits, noise, 2, host=True)
    assert fills == 2 and after == ''.join(T.tracking_lines(k, rows[k], mids[k], mhits[k]) for k in range(8))
    # --max-gap 0: nothing is filled, and the track falls into three segments
    track_results.main(common + ['--rts', '--max-gap', '0'] + KALMAN)
    assert len((tmp_path / 'tracks.txt').read_text().splitlines()) == 6
    # under the Kalman filter and the fourth metric too
    track_results.main(common[:2] + ['--metric', 'maha', '--threshold', '3', '--host', '--track-filter', 'kalman', '--rts'] + KALMAN)
    assert len((tmp_path / 'tracks.txt').read_text().splitlines()) == 8
    for bad in (['--rts'], ['--rts', '--smooth'] + KALMAN, ['--rts', '--max-gap', '-1'] + KALMAN, ['--max-gap', '1'],
                ['--rts'] + KALMAN[:-1] + ['0']):
        with pytest.raises(SystemExit):
            track_results.parse_args(common + bad)


def test_run_network_takes_the_smoother():
    from keras_retinanet_3D.bin import run_network
    common = ['synthetic:1234.h5', 'img', 'calib', 'planes', 'out', '--kitti', '--device-pose', '--track', 'dist', '--track-threshold', '3']
    args = run_network.parse_args(common + ['--track-rts'] + KALMAN)
    assert args.rts and args.max_gap == 2 and run_network.smoother_option(args) == (K.NOISE, 2)
    assert run_network.smoother_option(run_network.parse_args(common + ['--track-rts', '--track-max-gap', '1', '--track-max-age', '4'] + KALMAN)) == (K.NOISE, 1)
    assert run_network.smoother_option(run_network.parse_args(common)) is None
    assert run_network.track_option(args) == {'metric': 'dist', 'threshold': 3.0, 'max_age': 2, 'smooth': False}
    for bad in (['--track-rts'], ['--track-rts', '--track-smooth'] + KALMAN, ['--track-max-gap', '1'], ['--track-rts', '--track-max-gap', '-1'] + KALMAN):
        with pytest.raises(SystemExit):
            run_network.parse_args(common + bad)
    with pytest.raises(SystemExit):
        run_network.parse_args(['synthetic:1234.h5', 'img', 'calib', 'planes', 'out', '--kitti', '--device-pose', '--track-rts'] + KALMAN)
