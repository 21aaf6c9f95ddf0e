""" GPU tests of the offline smoother (csrc/track_smooth.hip, gpp_track_smooth_f64): the kernel against the NumPy
form (utils/track_smooth.py, itself held to the loop-written oracle by tests/test_track_smooth_cpu.py) on the rows, the fills and both
covariances -- every word ==, column 25 (an atan2) within 4 float32 ulp -- at the smallest shapes where the launches can go wrong. """
import numpy as np
import pytest
import torch

import track_smooth_cases as C
from track_oracle import padding, row
from keras_retinanet_3D.utils import track_smooth as S

pytestmark = pytest.mark.gpu
NOISE = C.NOISE


def device_equals_numpy(rows, index, ego=None, noise=NOISE):
    want = S.smooth_np(rows, index, noise, ego)
    got = S.smooth_device(rows, index, noise, ego)
    C.same_outputs(got, want)
    return got


@pytest.mark.parametrize('length', [1, 2, 3])
@pytest.mark.parametrize('n_seg', [1, 63, 64, 65])
def test_segment_counts_around_a_wavefront(n_seg, length):
    rows, ids = C.chains(n_seg, length)
    index = S.segments_of(ids, None, 0, rows)
    assert len(index.seg_frame) == n_seg and index.cell_row.size == n_seg * length
    got = device_equals_numpy(rows, index)
    assert (got[0].tobytes() == rows.tobytes()) == (length == 1)


def test_lanes_that_end_at_different_steps():
    """ one segment of 300 cells beside 64 of two cells: two blocks, the first with a pitch of 300 """
    rows = np.stack([padding(65) for _ in range(300)])
    ids = np.full((300, 65), -1, np.int32)
    for f in range(300):
        if f % 7 != 3 or f in (0, 299):
            rows[f, 0], ids[f, 0] = row(0.9, 1.0 + 0.05 * f + 0.3 * ((f * 7) % 5 - 2), 15.0 + 0.2 * f + ((f * 3) % 7 - 3), ry=0.01 * f - 1.5), 0
    short, short_ids = C.chains(64, 2)
    rows[100:102, 1:], ids[100:102, 1:] = short, short_ids + 1
    index = S.segments_of(ids, None, 1, rows)
    assert sorted(np.diff(index.seg_start).tolist()) == [2] * 64 + [300]
    got = device_equals_numpy(rows, index, C.records('yaw', 300))
    assert got[2].shape[0] == int((ids[:, 0] < 0).sum()) == 43


@pytest.mark.parametrize('G', [0, 1, 3])
def test_a_gap_of_exactly_max_gap(G):
    rows, ids = C.chains(5, 4, step=G + 1)
    index = S.segments_of(ids, None, G, rows)
    assert np.diff(index.seg_start).tolist() == [3 * G + 4] * 5
    assert device_equals_numpy(rows, index)[2].shape[0] == 15 * G


def test_a_frame_of_128_rows_all_in_segments():
    rows, ids = C.chains(128, 2)
    index = S.segments_of(ids, None, 0, rows)
    assert rows.shape == (2, 128, 36) and len(index.seg_frame) == 128
    got = device_equals_numpy(rows, index)
    assert (got[1][..., [0, 2]] > 0.0).all()


@pytest.mark.parametrize('kind', [None, 'identity', 'turns', 'general'])
def test_two_sequences_with_equal_ids_under_every_kind_of_record(kind):
    rows, ids = C.scene(11, N=24, D=6, cars=5, seq_start=[0, 10, 24], miss=0.3)
    index = S.segments_of(ids, [0, 10, 24], 2, rows)
    assert len(set(index.seg_id.tolist())) < len(index.seg_id)
    got = device_equals_numpy(rows, index, C.records(kind, 24))
    assert got[2].shape[0] >= 3


def test_in_place_without_covariances_and_on_tensors():
    rows, ids = C.scene(5, N=16, D=4, cars=4, miss=0.4)
    index = S.segments_of(ids, None, 3, rows)
    want = S.smooth_np(rows, index, NOISE)
    dev = torch.as_tensor(rows).cuda()
    out, row_cov, fills, fill_cov = S.smooth_device(dev, index, NOISE, out=dev, covariance=False)
    assert out.data_ptr() == dev.data_ptr() and row_cov is None and fill_cov is None and fills.shape[0] > 1
    C.same_outputs((out.cpu().numpy(), want[1], fills.cpu().numpy(), want[3]), want)
    fresh = torch.as_tensor(rows).cuda()
    res = S.smooth_device(fresh, index, NOISE)                            # out of place: the input keeps its bytes
    assert fresh.cpu().numpy().tobytes() == rows.tobytes()
    C.same_outputs(tuple(t.cpu().numpy() for t in res), want)


def test_nothing_to_smooth():
    rows, ids = C.chains(3, 2)
    nobody = S.segments_of(np.full_like(ids, -1), None, 1, rows)         # cells == 0
    assert nobody.cell_row.size == 0
    got = S.smooth_device(rows, nobody, NOISE)
    assert got[0].tobytes() == rows.tobytes() and not got[1].any() and got[1].shape == (2, 3, 3) and got[2].shape == (0, 36)
    for shape in ((0, 4, 36), (3, 0, 36)):                               # N * D == 0
        empty = np.zeros(shape, np.float32)
        index = S.segments_of(np.zeros(shape[:2], np.int32), None, 1, empty)
        got = S.smooth_device(empty, index, NOISE)
        assert got[0].shape == shape and got[1].shape == shape[:2] + (3,) and got[2].shape == (0, 36) and got[3].shape == (0, 3)


def test_the_order_of_the_segments_changes_no_output():
    rows, ids = C.scene(5, N=16, D=4, cars=4, miss=0.4)
    index = S.segments_of(ids, None, 3, rows)
    first = device_equals_numpy(rows, index)
    order = np.random.default_rng(0).permutation(len(index.seg_frame))
    second = device_equals_numpy(rows, S.reorder(index, order))
    assert np.array_equal(first[0], second[0], equal_nan=True) and np.array_equal(first[1], second[1])
    key = lambda f: sorted(map(bytes, f))  # noqa: E731
    assert key(first[2]) == key(second[2]) and key(first[3]) == key(second[3]) and first[2].shape[0] > 1


def test_a_restart_on_the_device():
    """ det not > 0 at one cell (tests/test_track_smooth_cpu.py): the cell restarts, the step into it is skipped, in the kernel too """
    noise = dict(NOISE, radial=(0.1, 1e150))
    rows = np.stack([padding(1) for _ in range(5)])
    for f, (x, z) in enumerate([(1e-3, 2e-3), (2e-3, 3e-3), (0.0, 1e6), (3e-3, 1e-3), (2e-3, 2e-3)]):
        rows[f, 0] = row(0.9, x, z)
    index = S.segments_of(np.zeros((5, 1), np.int32), None, 0, rows)
    device_equals_numpy(rows, index, noise=noise)


def test_track_results_on_the_device_writes_what_the_host_form_writes(tmp_path):
    """ bin/track_results.py --rts without --host against --host: the same lines; alpha, printed with two decimals behind an atan2, within
    one unit of its last digit """
    from keras_retinanet_3D.bin import track_results
    common = C.write_run(tmp_path)
    track_results.main(common + ['--rts'] + C.KALMAN)
    host = (tmp_path / 'tracks.txt').read_text().splitlines()
    track_results.main(common[:-1] + ['--rts'] + C.KALMAN)
    device = (tmp_path / 'tracks.txt').read_text().splitlines()
    assert len(host) == len(device) == 8
    for a, b in zip(host, device):
        a, b = a.split(), b.split()
        assert a[:5] == b[:5] and a[6:] == b[6:] and abs(float(a[5]) - float(b[5])) < 0.0101
