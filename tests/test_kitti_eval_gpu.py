""" KITTI's object benchmark on the GPU (csrc/kitti_eval.hip) against the loop-written oracle (tests/kitti_oracle.py):
the overlaps of every (detection, label) pair, the two passes of the matching, evaluate_kitti(device=True) against device=False, and
RetinaNet3D.score_poses_on_frames against the host form on the fetched rows.

Tolerance of the overlaps: coordinates up to 100 m and sides of at least 1 m in float64, with the device's cos / sin within an ulp of
libm's, leave about 1e-11 of absolute error in an area and less in a ratio: |kernel - oracle| <= 1e-9 on every finite entry, NaN exactly
where the oracle has NaN.  With r_y = 0 and dyadic coordinates every step is exact on both sides: equal.  The matching is compared
exactly; that is legitimate only while no overlap lies within rounding of min_overlap, which the stats test asserts on the oracle's
overlaps (the exactly dyadic 7/10 of case (vi) is the one allowed exception: it is equal on both sides). """
import ctypes
import math

import numpy as np
import pytest

import kitti_oracle as KO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import kitti_eval

pytestmark = pytest.mark.gpu
MIN_OVERLAP = (0.7, 0.7, 0.7)


def pack(images, D, A):
    """ [(rows (d, 36), labels (a, 16))] -> rows (B, D, 36) padded with -1 rows, labels (B, A, 16) zero-padded, counts (B,) """
    rows = np.full((len(images), D, 36), -1.0, np.float32)
    labels = np.zeros((len(images), A, 16), np.float64)
    counts = np.zeros(len(images), np.int32)
    for b, (r, g) in enumerate(images):
        r, g = np.asarray(r, np.float32).reshape(-1, 36), np.asarray(g, np.float64).reshape(-1, 16)
        rows[b, :r.shape[0]], labels[b, :g.shape[0]], counts[b] = r, g, g.shape[0]
    return rows, labels, counts


def on_device(*arrays):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(a)).to('cuda') for a in arrays]


def special_image():
    """ the pairs of the geometry test as one image: 2 x 2 squares and dyadic axis-aligned boxes as labels; as detections the quarter-turned
    square, the identical one, a contained one, one sharing an edge from outside, a disjoint one, two half a turn apart, rows with NaN
    3-D fields and padding rows in between """
    labels = [KO.make_label(hwl=(2.0, 2.0, 2.0), xyz=(0.0, 2.0, 10.0)),
              KO.make_label(hwl=(1.5, 2.0, 4.0), xyz=(8.0, 1.5, 12.0), box=(300.0, 100.0, 364.0, 148.0)),
              KO.make_label(hwl=(2.0, 2.0, 17.0), xyz=(30.0, 2.0, 20.0), box=(500.0, 100.0, 517.0, 160.0)),
              KO.make_label(kind=1, hwl=(1.75, 1.5, 3.25), xyz=(-9.0, 1.25, 25.5), ry=0.0, box=(10.0, 50.0, 90.5, 110.25)),
              KO.make_label(kind=2, hwl=(-1.0, -1.0, -1.0), xyz=(-1000.0, -1000.0, -1000.0), ry=-10.0, box=(600.0, 20.0, 900.0, 300.0)),
              KO.make_label(hwl=(1.6, 1.7, 4.1), xyz=(3.3, 1.6, 31.7), ry=0.6, box=(200.0, 120.0, 260.0, 170.0))]
    sq = dict(hwl=(2.0, 2.0, 2.0), box=(100.0, 100.0, 200.0, 160.0))
    rows = [KO.make_row(0.9, xyz=(0.0, 2.0, 10.0), ry=math.pi / 4, **sq), KO.make_row(0.8, xyz=(0.0, 2.0, 10.0), **sq),
            KO.make_row(0.7, hwl=(1.0, 1.0, 1.0), xyz=(0.25, 1.5, 10.25), box=(120.0, 110.0, 180.0, 150.0)),
            KO.padding_row(),
            KO.make_row(0.6, xyz=(2.0, 2.0, 10.0), **sq), KO.make_row(0.5, xyz=(5.0, 2.0, 11.0), ry=0.7, **sq),
            KO.make_row(0.45, hwl=(1.6, 1.7, 4.1), xyz=(3.5, 1.6, 31.5), ry=0.5, box=(202.0, 121.0, 262.0, 169.0)),
            KO.make_row(0.44, hwl=(1.6, 1.7, 4.1), xyz=(3.5, 1.6, 31.5), ry=0.5 + math.pi, box=(202.0, 121.0, 262.0, 169.0)),
            KO.make_row(0.4, hwl=(1.5, 2.0, 4.0), xyz=(8.5, 1.75, 12.25), box=(308.0, 104.0, 372.0, 152.0)),
            KO.make_row(0.35, hwl=(2.0, 2.0, 17.0), xyz=(33.0, 2.0, 20.0), box=(503.0, 100.0, 520.0, 160.0)),
            KO.make_row(0.3, box=(700.0, 100.0, 800.0, 160.0), xyz=(50.0, 1.5, 50.0))]
    for k in (1, 8):
        nan_row = rows[k].copy()
        nan_row[19:26], nan_row[30:33], nan_row[12] = np.nan, np.nan, 0.33
        rows.append(nan_row)
    rows.append(KO.padding_row())
    return np.array(rows, np.float32), np.array(labels, np.float64)


def dyadic_image():
    """ r_y = 0 and coordinates in quarters: every step of every plane is exact """
    rng = np.random.default_rng(31)
    q = lambda lo, hi: float(rng.integers(int(lo * 4), int(hi * 4) + 1)) / 4.0  # noqa: E731
    labels, rows = [], []
    for _ in range(8):
        x1, y1 = q(0, 600), q(50, 200)
        labels.append(KO.make_label(box=(x1, y1, x1 + q(20, 100), y1 + q(20, 100)), hwl=(q(1, 2), q(1, 3), q(2, 6)), xyz=(q(-6, 6), q(1, 2), q(8, 16))))
    for k in range(24):
        g = labels[k % 8]
        rows.append(KO.make_row(q(0, 1), box=(g[4] + q(-8, 8), g[5] + q(-8, 8), g[6] + q(-8, 8), g[7] + q(-8, 8)), hwl=(q(1, 2), q(1, 3), q(2, 6)),
                                xyz=(g[11] + q(-2, 2), g[12] + q(-0.5, 0.5), g[13] + q(-2, 2))))
    return np.array(rows, np.float32), np.array(labels, np.float64)


def crowd_image():
    """ 30 detections on 5 labels with tied scores """
    rng = np.random.default_rng(32)
    labels = [KO.make_label(box=(100.0 + 150 * k, 100.0, 200.0 + 150 * k, 160.0), xyz=(-20.0 + 8 * k, 1.5, 20.0), occ=k % 3, ry=0.2 * k) for k in range(5)]
    rows = []
    for k in range(30):
        g = labels[k % 5]
        rows.append(KO.row_like(g, [0.9, 0.9, 0.6, 0.6, 0.6, 0.3][k // 5], box=(g[4] + rng.uniform(-6, 6), g[5] + rng.uniform(-4, 4), g[6] + rng.uniform(-6, 6),
                                g[7] + rng.uniform(-4, 4)), xyz=(g[11] + rng.uniform(-0.25, 0.25), g[12], g[13] + rng.uniform(-0.12, 0.12)),
                                alpha=g[3] + rng.uniform(-1, 1)))
    return np.array(rows, np.float32), np.array(labels, np.float64)


def cases_image():
    """ cases (iii) - (x) of tests/test_kitti_eval_cpu.py in one image: every case has its own place in the image and on the ground """
    def at(k, **kw):
        kw.setdefault('box', (100.0 + 150 * k, 100.0, 200.0 + 150 * k, 160.0))
        kw.setdefault('xyz', (-150.0 + 30 * k, 1.5, 20.0))
        return KO.make_label(**kw)

    labels = [at(0), at(1, kind=1), KO.make_label(kind=2, box=(100.0, 300.0, 400.0, 370.0), hwl=(-1.0, -1.0, -1.0), xyz=(-1000.0, -1000.0, -1000.0), ry=-10.0),
              at(3, box=(550.0, 100.0, 650.0, 130.0)),
              at(4, box=(700.0, 100.0, 717.0, 160.0), hwl=(2.0, 2.0, 17.0), xyz=(-30.0, 2.0, 20.0)),
              at(5, box=(850.0, 100.0, 868.0, 160.0), hwl=(2.0, 2.0, 18.0), xyz=(0.0, 2.0, 20.0)),
              at(6), at(7), at(8), at(9, alpha=0.5)]
    g = labels
    rows = [KO.row_like(g[0], 0.95),
            KO.row_like(g[1], 0.9),                                                                   # (iii) on the Van
            KO.make_row(0.85, box=(150.0, 310.0, 250.0, 360.0), xyz=(200.0, 1.5, 60.0)),              # (iv) in the DontCare box
            KO.row_like(g[3], 0.8),                                                                   # (v) 30 pixels high
            KO.row_like(g[4], 0.75, box=(703.0, 100.0, 720.0, 160.0), xyz=(-27.0, 2.0, 20.0)),        # (vi) exactly 7/10
            KO.row_like(g[5], 0.7, box=(852.0, 100.0, 870.0, 160.0), xyz=(2.0, 2.0, 20.0)),           # (vi) exactly 8/10
            KO.row_like(g[6], 0.65),                                                                  # (vii) NaN 3-D fields (set below)
            KO.row_like(g[7], 0.3, box=(1150.0, 100.0, 1250.0, 120.0)),                               # (viii) too low, first in row order
            KO.row_like(g[7], 0.6, xyz=(60.1, 1.5, 20.0)),                                            # (viii) the one that counts
            KO.row_like(g[8], 0.55, box=(1304.0, 100.0, 1404.0, 160.0), xyz=(90.3, 1.5, 20.0)),       # (ix) loose, the higher score
            KO.row_like(g[8], 0.5),                                                                   # (ix) tight
            KO.row_like(g[9], 0.4, alpha=0.5), KO.row_like(g[9], 0.4, alpha=2.0),                     # (x) equal scores
            KO.make_row(0.2, box=(50.0, 500.0, 150.0, 560.0), xyz=(300.0, 1.5, 80.0))]                # the lowest threshold's false positive
    rows[6][19:26], rows[6][30:33] = np.nan, np.nan
    return np.array(rows, np.float32), np.array(labels, np.float64)


def big_image():
    """ D = A = 128: 128 labels (one in five counts, the others are of another type, Vans or DontCare) and 128 detections """
    rng = np.random.default_rng(33)
    rows, labels = KO.random_scene(rng, 128, 128)
    labels[:, 0] = np.where(np.arange(128) % 5 == 0, 0.0, np.where(np.arange(128) % 5 == 1, labels[:, 0], 3.0))
    return rows, labels


class Batch(object):
    """ some images packed to (D, A), the oracle's overlaps and the kernel's """

    def __init__(self, images, D, A):
        self.images, self.D, self.A = images, D, A
        self.rows, self.labels, self.counts = pack(images, D, A)
        self.want = np.zeros((len(images), 4, D, A))
        for b, (r, g) in enumerate(images):
            o = KO.image_overlaps(r, g)
            self.want[b, :, :o.shape[1], :o.shape[2]] = o
        self.dev = on_device(self.rows, self.labels, self.counts)
        self.overlaps = hip.kitti_overlaps(*self.dev)

    def padded(self, b):
        """ image b as the kernel sees it: D rows, its own labels """
        return self.rows[b], self.labels[b, :self.counts[b]], self.want[b][:, :, :self.counts[b]]


@pytest.fixture(scope='module')
def small():
    rng = np.random.default_rng(30)
    images = [special_image(), KO.random_scene(rng, 12, 40), KO.random_scene(rng, 7, 33), dyadic_image(), crowd_image(), cases_image(),
              (KO.random_scene(rng, 3, 9)[0], np.zeros((0, 16))), (np.zeros((0, 36), np.float32), KO.random_scene(rng, 5, 2)[1])]
    return Batch(images, 40, 12)                     # 480 pairs: the overlaps are staged in LDS


@pytest.fixture(scope='module')
def big():
    return Batch([cases_image(), big_image(), crowd_image()], 128, 128)          # 16 384 pairs: read from global memory


# ---------------------------------------------------------------------------------------------------- overlaps
def check_overlaps(batch):
    got = batch.overlaps.cpu().numpy()
    assert got.shape == batch.want.shape
    assert np.array_equal(np.isnan(got), np.isnan(batch.want))
    worst = float(np.nanmax(np.abs(got - batch.want)))
    print('overlaps: worst |kernel - oracle| = {:.3e} over {} finite entries, {} NaN'.format(worst, int(np.isfinite(got).sum()), int(np.isnan(got).sum())))
    assert worst <= 1e-9
    return got


def test_overlaps_against_the_oracle(small):
    got = check_overlaps(small)
    want = small.want
    # image 0: the special pairs, against label 0 (the 2 x 2 square at the origin of its place)
    assert abs(want[0, 1, 0, 0] - 8 * (math.sqrt(2) - 1) / (8 - 8 * (math.sqrt(2) - 1))) <= 1e-12
    assert got[0, 1, 1, 0] == 1.0 and got[0, 2, 1, 0] == 1.0 and got[0, 0, 1, 0] == 1.0           # identical
    assert got[0, 1, 2, 0] == 0.25 and got[0, 2, 2, 0] == 0.125                                    # contained: the ratio of the areas, of the volumes
    assert got[0, 1, 4, 0] == 0.0 and got[0, 1, 5, 0] == 0.0                                       # an edge shared from outside; disjoint
    assert abs(got[0, 1, 6, 5] - got[0, 1, 7, 5]) <= 1e-6 and got[0, 1, 6, 5] > 0.5                 # half a turn apart (r_y is a float32)
    assert (got[0, 0:3, 9, 2] == 0.7).all()                                                        # exactly 7/10 in every metric
    assert (got[0, :, 3] == 0).all() and (got[0, :, 13:] == 0).all() and (got[0, :, :, 6:] == 0).all()      # padding rows, labels beyond the count
    assert np.isnan(got[0, 1:3, 11:13, :6]).all() and not np.isnan(got[0, [0, 3], 11:13]).any()             # NaN 3-D fields: the image planes stay
    assert np.isnan(want).sum() > 0 and (small.counts < small.A).any()
    # image 3: r_y = 0 and dyadic coordinates: equal, and the BEV plane is the image formula on the ground rectangle
    assert np.array_equal(got[3], want[3]) and (got[3, 1] > 0).sum() > 10
    rows, labels = small.images[3]
    for d in range(rows.shape[0]):
        for a in range(labels.shape[0]):
            box = lambda h, w, l, x, y, z: (x - l / 2.0, z - w / 2.0, x + l / 2.0, z + w / 2.0)  # noqa: E731
            det = box(float(rows[d, 30]), float(rows[d, 17]), float(rows[d, 18]), float(rows[d, 19]), float(rows[d, 31]), float(rows[d, 21]))
            assert got[3, 1, d, a] == KO.image_iou(det, box(*labels[a, 8:14]))


def test_overlaps_at_the_largest_shape(big):
    check_overlaps(big)


# ---------------------------------------------------------------------------------------------------- stats
def oracle_passes(batch):
    """ pass 1, the thresholds of the batch, pass 2 -- all by the oracle, on ITS overlaps """
    B, A = len(batch.images), batch.A
    tp_scores = np.full((B, 3, 3, A), np.nan, np.float32)
    n_gt = np.zeros((B, 3, 3), np.int32)
    thr = np.zeros((3, 3, 41), np.float32)
    n_thr = np.zeros((3, 3), np.int32)
    stats = np.zeros((B, 3, 3, 41, 3), np.int32)
    sim = np.zeros((B, 3, 3, 41))
    for m in range(3):
        for d in range(3):
            for b in range(B):
                rows, labels, ov = batch.padded(b)
                one = KO.match(rows, labels, ov, m, d, MIN_OVERLAP[m])
                tp_scores[b, m, d, :labels.shape[0]], n_gt[b, m, d] = one['tp_scores'], one['n_gt']
            v = tp_scores[:, m, d].ravel()
            t = KO.thresholds(v[~np.isnan(v)], n_gt[:, m, d].sum()) if n_gt[:, m, d].sum() else []
            thr[m, d, :len(t)], n_thr[m, d] = t, len(t)
            for k in range(len(t)):
                for b in range(B):
                    rows, labels, ov = batch.padded(b)
                    one = KO.match(rows, labels, ov, m, d, MIN_OVERLAP[m], t[k])
                    stats[b, m, d, k], sim[b, m, d, k] = (one['tp'], one['fp'], one['fn']), one['similarity']
    return tp_scores, n_gt, thr, n_thr, stats, sim


def no_overlap_near_the_minimum(batch, exact_allowed_in):
    """ the condition of the exact comparison: on the ORACLE's overlaps no finite entry lies within 1e-6 of min_overlap, but for the
    exactly dyadic 7/10 (equal on both sides: test_overlaps_against_the_oracle) """
    for b in range(len(batch.images)):
        near = np.isfinite(batch.want[b]) & (np.abs(batch.want[b] - 0.7) < 1e-6)
        if near.any():
            assert b in exact_allowed_in and (batch.want[b][near] == 0.7).all(), (b, batch.want[b][near])


def check_stats(batch, exact_allowed_in):
    no_overlap_near_the_minimum(batch, exact_allowed_in)
    tp_scores, n_gt, thr, n_thr, stats, sim = oracle_passes(batch)
    got_scores, got_n = hip.kitti_stats(*batch.dev, batch.overlaps, MIN_OVERLAP)
    assert np.array_equal(got_scores.cpu().numpy(), tp_scores, equal_nan=True)
    assert np.array_equal(got_n.cpu().numpy(), n_gt)
    thr_d, n_thr_d = on_device(thr, n_thr)
    got_stats, got_sim = hip.kitti_stats(*batch.dev, batch.overlaps, MIN_OVERLAP, thr_d, n_thr_d)
    got_stats, got_sim = got_stats.cpu().numpy(), got_sim.cpu().numpy()
    assert np.array_equal(got_stats, stats)
    assert np.array_equal(np.isnan(got_sim), np.isnan(sim))
    worst = float(np.nanmax(np.abs(got_sim - sim)))
    print('stats: {} thresholds, {} tp at the last of each bin, worst similarity difference {:.3e}'.format(
        int(n_thr.sum()), int(sum(stats[:, m, d, n_thr[m, d] - 1, 0].sum() for m in range(3) for d in range(3) if n_thr[m, d])), worst))
    assert worst <= 1e-9
    # a shorter table (T < 41) gives the same columns
    T = max(1, int(n_thr.max()) - 1)
    short_thr, short_n = on_device(np.ascontiguousarray(thr[:, :, :T]), np.minimum(n_thr, T).astype(np.int32))
    short_stats, _ = hip.kitti_stats(*batch.dev, batch.overlaps, MIN_OVERLAP, short_thr, short_n)
    assert np.array_equal(short_stats.cpu().numpy(), stats[:, :, :, :T])
    return n_gt, n_thr, stats


def test_stats_against_the_oracle(small):
    n_gt, n_thr, stats = check_stats(small, exact_allowed_in=(0, 5))
    assert (n_thr > 3).all() and n_gt[6].sum() == 0 and n_gt[7].sum() > 0
    # the image without labels: every detection above the threshold and high enough is a false positive; the one without detections: misses
    assert stats[6, 0, 1, n_thr[0, 1] - 1, 1] > 0 and stats[6, :, :, :, [0, 2]].sum() == 0
    assert stats[7, 0, 2, 0, 2] == n_gt[7, 0, 2] and stats[7, :, :, :, :2].sum() == 0


def test_stats_at_the_largest_shape(big):
    n_gt, n_thr, stats = check_stats(big, exact_allowed_in=(0,))
    assert n_gt[1, 0, 2] > 10 and (n_thr > 3).all()


def test_stats_without_labels_and_limits():
    import torch
    rng = np.random.default_rng(34)
    rows = np.stack([KO.random_scene(rng, 2, 9)[0] for _ in range(2)])
    rows[0, :, 12] = np.linspace(0.9, 0.1, 9)
    rows_d, = on_device(rows)
    labels_d = torch.zeros((2, 0, 16), dtype=torch.float64, device='cuda')
    counts_d = torch.zeros((2,), dtype=torch.int32, device='cuda')
    overlaps = hip.kitti_overlaps(rows_d, labels_d, counts_d)
    assert tuple(overlaps.shape) == (2, 4, 9, 0)
    scores, n_gt = hip.kitti_stats(rows_d, labels_d, counts_d, overlaps, MIN_OVERLAP)
    assert tuple(scores.shape) == (2, 3, 3, 0) and not n_gt.cpu().numpy().any()
    thr = np.zeros((3, 3, 2), np.float32)
    thr[:, :, 0], thr[:, :, 1] = 0.5, 0.05
    thr_d, n_d = on_device(thr, np.full((3, 3), 2, np.int32))
    stats, sim = hip.kitti_stats(rows_d, labels_d, counts_d, overlaps, MIN_OVERLAP, thr_d, n_d)
    stats = stats.cpu().numpy()
    for b in range(2):
        for d in range(3):
            high = np.abs(rows[b, :, 29].astype(np.float64) - rows[b, :, 27]) >= (40, 25, 25)[d]
            for k in range(2):
                assert stats[b, :, d, k].tolist() == [[0, int((high & ~(rows[b, :, 12] < thr[0, 0, k])).sum()), 0]] * 3
    assert not sim.cpu().numpy().any()
    # limits, on the device's pointers
    big_rows = torch.full((1, 129, 36), -1.0, dtype=torch.float32, device='cuda')
    with pytest.raises(hip.GppError, match='GPP_ERR_UNSUPPORTED'):
        hip.kitti_overlaps(big_rows, torch.zeros((1, 4, 16), dtype=torch.float64, device='cuda'), counts_d[:1])
    with pytest.raises(hip.GppError, match='GPP_ERR_UNSUPPORTED'):
        hip.kitti_overlaps(rows_d[:1], torch.zeros((1, 129, 16), dtype=torch.float64, device='cuda'), counts_d[:1])
    with pytest.raises(hip.GppError, match='GPP_ERR_BAD_ARG'):
        hip.kitti_stats(rows_d, labels_d, counts_d, overlaps, MIN_OVERLAP, torch.zeros((3, 3, 42), dtype=torch.float32, device='cuda'), n_d)
    mo = (ctypes.c_double * 3)(*MIN_OVERLAP)
    p = ctypes.c_void_p(rows_d.data_ptr())
    assert hip.lib().gpp_kitti_overlaps_f64(None, p, p, 2, 9, 4, p, None) == -1
    assert hip.lib().gpp_kitti_stats_f64(p, p, p, p, mo, None, None, 2, 9, 4, 0, p, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------- end to end
def assert_same_result(got, want):
    assert set(got) == set(want)
    for key, entry in want.items():
        for name, value in entry.items():
            if name.startswith('aos'):
                assert got[key][name] == pytest.approx(value, abs=1e-9, nan_ok=True), (key, name)
            else:
                assert np.array_equal(got[key][name], value), (key, name, got[key][name], value)          # integers, thresholds, AP: equal


def test_evaluate_kitti_on_the_device_is_the_host_form(tmp_path, monkeypatch):
    label_dir, result_dir = KO.write_dataset(tmp_path, n=6, seed=35)
    want = kitti_eval.evaluate_kitti(label_dir, result_dir)
    assert_same_result(kitti_eval.evaluate_kitti(label_dir, result_dir, device=True), want)
    assert sum(len(want[(m, 'hard')]['thresholds']) for m in kitti_eval.METRICS) > 6
    # several chunks give what one gives
    monkeypatch.setattr(kitti_eval, 'OVERLAP_WORKSPACE_BYTES', 2 * 4 * 12 * 6 * 8)
    assert kitti_eval.chunk_images(12, 6) == 2
    assert_same_result(kitti_eval.evaluate_kitti(label_dir, result_dir, device=True), want)


def test_score_poses_on_frames_is_the_host_form_on_the_fetched_rows(monkeypatch):
    from keras_retinanet_3D import models
    from keras_retinanet_3D.utils import synthetic
    from keras_retinanet_3D.utils.image import compute_resize_scale
    monkeypatch.setenv('GPP_AUTOTUNE', '0')                          # (a tile never changes a byte: tests/test_network_gpu.py)
    model = models.load_model('synthetic:3', backbone_name='resnet50', dtype='f32', pose=True)
    B, h, w = 2, 96, 320
    frames = np.stack([(np.random.default_rng(36 + k).integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8) for k in range(B)])
    P_inv = np.stack([synthetic.synthetic_calibration(compute_resize_scale((h, w, 3)))[1]] * B).astype(np.float32)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    (rows, counts), _ = model.predict_poses_on_frames(frames, P_inv, planes)
    assert counts.min() > 0
    # labels from the model's own rows, jittered: every fourth detection with finite 3-D fields, as a Car, a Van or a DontCare region
    rng = np.random.default_rng(37)
    labels = []
    for b in range(B):
        labels.append([])
        for d in range(0, int(counts[b]), 4):
            r = rows[b, d].astype(np.float64)
            if not np.isfinite(r).all():
                continue
            box = r[26:30] + rng.uniform(-1.5, 1.5, 4)
            labels[-1].append(KO.make_label(kind=(0, 0, 0, 1, 2)[len(labels[-1]) % 5], box=box, hwl=(r[30] * 1.02, r[17] * 0.99, r[18] * 1.01),
                                            xyz=(r[19] + rng.uniform(-0.1, 0.1), r[31], r[21] + rng.uniform(-0.1, 0.1)), ry=r[32] + 0.02, alpha=r[25] + 0.1))
        labels[-1] = np.array(labels[-1], np.float64).reshape(-1, 16)
    assert sum(g.shape[0] for g in labels) > 4
    chunk, _ = model.score_poses_on_frames(frames, P_inv, planes, labels)
    assert chunk.rows.cpu().numpy().tobytes() == rows.tobytes()
    got = chunk.overlaps.cpu().numpy()
    for b in range(B):
        want = kitti_eval.image_overlaps(rows[b], labels[b])
        assert np.array_equal(np.isnan(got[b][:, :, :want.shape[2]]), np.isnan(want))
        assert np.nanmax(np.abs(got[b][:, :, :want.shape[2]] - want)) <= 1e-9
    assert_same_result(kitti_eval.evaluate_chunks([chunk]), kitti_eval.evaluate_rows(list(rows), labels))
    # the plan's next run does not reach into the chunk
    model.predict_poses_on_frames(frames[::-1].copy(), P_inv, planes)
    assert chunk.rows.cpu().numpy().tobytes() == rows.tobytes()
    with pytest.raises(ValueError):
        model.score_poses_on_frames(frames, P_inv, planes, labels[:1])
