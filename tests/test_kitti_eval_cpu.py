""" KITTI's object benchmark without a GPU: the oracle's geometry (tests/kitti_oracle.py) against an independent
construction with scipy, the rules on hand-built cases -- each on the host form (utils/kitti_eval.py, device=False) and on the oracle --,
the file parsers, the command line, and what the device entry points refuse on the host. """
import ctypes
import json
import math
import os

import numpy as np
import pytest

import kitti_oracle as KO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import gpp_utils, kitti_eval

METRICS, DIFFS = kitti_eval.METRICS, kitti_eval.DIFFICULTIES


# ---------------------------------------------------------------------------------------------------- geometry
def scipy_intersection(box0, box1):
    """ the intersection area of two placed rectangles as the hull of the intersection of their eight half-planes """
    from scipy.optimize import linprog
    from scipy.spatial import ConvexHull, HalfspaceIntersection
    planes = []
    for box in (box0, box1):
        c = KO.box_corners(*box)
        for k in range(4):
            (ax, az), (bx, bz) = c[k], c[(k + 1) % 4]
            nx, nz = (bz - az), -(bx - ax)                    # outward normal of a counter-clockwise polygon
            n = math.hypot(nx, nz)
            planes.append([nx / n, nz / n, -(nx * ax + nz * az) / n])
    planes = np.array(planes)
    # the deepest interior point (Chebyshev centre); no interior: no area
    res = linprog([0, 0, -1], A_ub=np.hstack([planes[:, :2], np.ones((8, 1))]), b_ub=-planes[:, 2], bounds=[(None, None)] * 2 + [(0, None)])
    if not res.success or res.x[2] < 1e-9:
        return 0.0
    points = HalfspaceIntersection(planes, res.x[:2]).intersections
    return ConvexHull(points).volume


def test_the_oracles_bev_intersection_agrees_with_scipy_on_200_pairs():
    rng = np.random.default_rng(20)
    worst = 0.0
    for _ in range(200):
        a = (rng.uniform(3, 5), rng.uniform(1.5, 2), rng.uniform(-10, 10), rng.uniform(5, 40), rng.uniform(-math.pi, math.pi))
        b = (rng.uniform(3, 5), rng.uniform(1.5, 2), a[2] + rng.uniform(-3, 3), a[3] + rng.uniform(-3, 3), rng.uniform(-math.pi, math.pi))
        worst = max(worst, abs(KO.bev_intersection(*(a + b)) - scipy_intersection(a, b)))
    assert worst <= 1e-9, worst


def test_special_pairs():
    sq = (2.0, 2.0, 0.0, 0.0, 0.0)
    assert abs(KO.bev_intersection(*(sq + (2.0, 2.0, 0.0, 0.0, math.pi / 4))) - 8 * (math.sqrt(2) - 1)) <= 1e-12
    assert KO.bev_iou(*(sq + sq)) == 1.0
    assert KO.bev_iou(*((4.0, 2.0, 1.0, 3.0, 0.0) + (2.0, 1.0, 1.5, 3.25, 0.0))) == 2.0 / 8.0              # contained: the ratio of the areas
    assert abs(KO.bev_iou(*((4.0, 2.0, 1.0, 3.0, 0.3) + (2.0, 1.0, 1.0, 3.0, 0.3))) - 0.25) <= 1e-12
    assert KO.bev_iou(*(sq + (2.0, 2.0, 2.0, 0.0, 0.0))) == 0.0                                            # an edge shared from outside
    assert KO.bev_iou(*(sq + (2.0, 2.0, 5.0, 1.0, 0.7))) == 0.0                                            # disjoint
    a, b = (4.2, 1.7, 0.3, 10.0, 0.4), (3.9, 1.6, 0.9, 10.4, -1.1)
    assert abs(KO.bev_iou(*(a + b)) - KO.bev_iou(*(a[:4] + (a[4] + math.pi,) + b[:4] + (b[4] + math.pi,)))) <= 1e-12
    # axis-aligned: the image formula on (x - l/2, z - w/2, x + l/2, z + w/2)
    for (l0, w0, x0, z0), (l1, w1, x1, z1) in (((4, 2, 0, 0), (3, 2, 1, 0.5)), ((5, 1.5, 2, 7), (4, 2, 3.25, 7.5)), ((4, 2, 0, 0), (4, 2, 9, 9))):
        box = lambda l, w, x, z: (x - l / 2.0, z - w / 2.0, x + l / 2.0, z + w / 2.0)  # noqa: E731
        assert KO.bev_iou(l0, w0, x0, z0, 0.0, l1, w1, x1, z1, 0.0) == KO.image_iou(box(l0, w0, x0, z0), box(l1, w1, x1, z1))


def test_the_host_forms_overlaps_are_the_oracles():
    rng = np.random.default_rng(21)
    rows, labels = KO.random_scene(rng, 9, 25)
    rows[3, 19:26], rows[3, 30:33] = np.nan, np.nan          # a singular pose: NaN 3-D fields
    rows[7] = -1.0                                            # a padding row
    want, got = KO.image_overlaps(rows, labels), kitti_eval.image_overlaps(rows, labels)
    assert np.array_equal(np.isnan(want), np.isnan(got))
    assert np.isnan(want[1:3, 3]).all() and not np.isnan(want[[0, 3]][:, 3]).any() and (want[:, 7] == 0).all()
    assert np.nanmax(np.abs(want - got)) <= 1e-12


# ---------------------------------------------------------------------------------------------------- rules
def both(rows_list, labels_list, min_overlap=(0.7, 0.7, 0.7)):
    """ the host form's result and the oracle's, after checking that they agree """
    rows_list = [np.asarray(r, np.float32).reshape(-1, 36) for r in rows_list]
    labels_list = [np.asarray(g, np.float64).reshape(-1, 16) for g in labels_list]
    host = kitti_eval.evaluate_rows(rows_list, labels_list, min_overlap)
    oracle = KO.evaluate(rows_list, labels_list, min_overlap)
    for m, metric in enumerate(METRICS):
        for d, diff in enumerate(DIFFS):
            h, o = host[(metric, diff)], oracle[(m, d)]
            assert [float(t) for t in h['thresholds']] == o['thresholds'], (metric, diff)
            for k in ('tp', 'fp', 'fn'):
                assert list(h[k]) == o[k], (metric, diff, k)
            for k in ('ap_r40', 'ap_r11'):
                assert h[k] == pytest.approx(o[k], abs=1e-9), (metric, diff, k)
            if m == 0:
                for k in ('aos_r40', 'aos_r11'):
                    assert host[('aos', diff)][k] == pytest.approx(o[k], abs=1e-9, nan_ok=True), (diff, k)
    return host


def spread_labels(n, **kw):
    """ n Car labels that do not overlap one another in any metric """
    return [KO.make_label(box=(100.0 + 150 * k, 100.0, 200.0 + 150 * k, 160.0), xyz=(-20.0 + 8 * k, 1.5, 20.0), **kw) for k in range(n)]


def test_i_every_label_matched_and_no_fp_gives_100():
    # 41 labels that count: every true positive's score is a threshold, so the 41 recall points are all reached
    labels = [spread_labels(11), spread_labels(10), spread_labels(10), spread_labels(10)]
    rows, score = [], 0.99
    for image in labels:
        rows.append([])
        for g in image:
            rows[-1].append(KO.row_like(g, score))
            score -= 0.02
    res = both(rows, labels)
    for key, entry in res.items():
        for name in ('ap_r40', 'ap_r11', 'aos_r40', 'aos_r11'):
            if name in entry:
                assert entry[name] == pytest.approx(100.0, abs=1e-9), (key, name)
        if 'tp' in entry:
            assert len(entry['thresholds']) == 41 and int(entry['tp'][-1]) == 41 and not np.any(entry['fp']) and int(entry['fn'][-1]) == 0


def test_ii_the_worked_example():
    labels = spread_labels(4)
    rows = [KO.row_like(labels[0], 0.9), KO.make_row(0.8, box=(800.0, 200.0, 900.0, 260.0), xyz=(15.0, 1.5, 50.0)), KO.row_like(labels[1], 0.7)]
    res = both([rows], [labels])
    for metric in METRICS:
        e = res[(metric, 'easy')]
        assert [float(t) for t in e['thresholds']] == [float(np.float32(0.9)), float(np.float32(0.7))]
        assert (list(e['tp']), list(e['fp']), list(e['fn'])) == ([1, 2], [0, 1], [3, 2])
        assert e['ap_r40'] == pytest.approx(100.0 * (2.0 / 3.0) / 40.0, abs=1e-12)
        assert e['ap_r11'] == pytest.approx(100.0 / 11.0, abs=1e-12)


def test_iii_a_van_matched_by_a_detection_is_neither_tp_nor_fp():
    labels = spread_labels(2)
    labels[1][0] = 1.0
    res = both([[KO.row_like(labels[0], 0.9), KO.row_like(labels[1], 0.8)]], [labels])
    for metric in METRICS:
        e = res[(metric, 'easy')]
        assert (list(e['tp']), list(e['fp']), list(e['fn'])) == ([1], [0], [0])


def test_iv_a_detection_in_a_dontcare_box_is_no_fp_for_the_image_metric_only():
    labels = spread_labels(1) + [KO.make_label(kind=2, box=(600.0, 50.0, 900.0, 300.0), hwl=(-1.0, -1.0, -1.0), xyz=(-1000.0, -1000.0, -1000.0), ry=-10.0)]
    rows = [KO.row_like(labels[0], 0.5), KO.make_row(0.9, box=(700.0, 100.0, 800.0, 160.0), xyz=(15.0, 1.5, 50.0))]
    res = both([rows], [labels])
    assert list(res[('image', 'easy')]['fp']) == [0]
    assert list(res[('bev', 'easy')]['fp']) == [1] and list(res[('3d', 'easy')]['fp']) == [1]


def test_v_thirty_pixels_count_at_moderate_and_are_ignored_at_easy():
    labels = [KO.make_label(box=(100.0, 100.0, 200.0, 130.0))]
    res = both([[KO.row_like(labels[0], 0.9)]], [labels])
    for metric in METRICS:
        assert len(res[(metric, 'easy')]['thresholds']) == 0 and res[(metric, 'easy')]['ap_r40'] == 0.0
        for diff in ('moderate', 'hard'):
            assert list(res[(metric, diff)]['tp']) == [1] and res[(metric, diff)]['ap_r11'] == pytest.approx(100.0 / 11.0)


def exact_pair(shift):
    """ 10-long boxes shifted by `shift` along x (image) and along the length (BEV, 3-D): IoU (10 - s) / (10 + s), exactly """
    label = KO.make_label(box=(100.0, 100.0, 110.0, 160.0), hwl=(2.0, 2.0, 10.0), xyz=(0.0, 2.0, 20.0))
    row = KO.row_like(label, 0.9, box=(100.0 + shift, 100.0, 110.0 + shift, 160.0), xyz=(float(shift), 2.0, 20.0))
    return row, label


def test_vi_an_overlap_of_exactly_the_minimum_is_no_match():
    # two 17-wide intervals offset by 3 share 14 of 20: exactly 7/10
    label = KO.make_label(box=(100.0, 100.0, 117.0, 160.0), hwl=(2.0, 2.0, 17.0), xyz=(0.0, 2.0, 20.0))
    row = KO.row_like(label, 0.9, box=(103.0, 100.0, 120.0, 160.0), xyz=(3.0, 2.0, 20.0))
    ov = KO.image_overlaps([row], [label])
    assert (ov[:3, 0, 0] == 0.7).all() and (kitti_eval.image_overlaps([row], [label])[:3, 0, 0] == 0.7).all()
    res = both([[row]], [[label]])
    for metric in METRICS:
        assert len(res[(metric, 'easy')]['thresholds']) == 0
    # two 18-wide intervals offset by 2 share 16 of 20: exactly 8/10
    label = KO.make_label(box=(100.0, 100.0, 118.0, 160.0), hwl=(2.0, 2.0, 18.0), xyz=(0.0, 2.0, 20.0))
    row = KO.row_like(label, 0.9, box=(102.0, 100.0, 120.0, 160.0), xyz=(2.0, 2.0, 20.0))
    assert (KO.image_overlaps([row], [label])[:3, 0, 0] == 0.8).all()
    res = both([[row]], [[label]])
    for metric in METRICS:
        assert list(res[(metric, 'easy')]['tp']) == [1]


def test_vii_a_row_with_nan_3d_fields_matches_in_the_image_metric_only():
    labels = spread_labels(1)
    row = KO.row_like(labels[0], 0.9)
    row[19:26], row[30:33] = np.nan, np.nan
    res = both([[row]], [labels])
    assert list(res[('image', 'easy')]['tp']) == [1]
    for metric in ('bev', '3d'):
        assert len(res[(metric, 'easy')]['thresholds']) == 0 and res[(metric, 'easy')]['ap_r40'] == 0.0


def test_viii_an_ignored_detection_is_displaced_by_a_later_one_that_counts():
    # Moderate: a 20-pixel-high detection (too low: status 1) comes first and overlaps by more than the minimum is impossible in the image
    # metric with so different a height, so the case is built for BEV / 3-D, whose overlap does not read the box
    labels = spread_labels(1)
    low = KO.row_like(labels[0], 0.9, box=(100.0, 100.0, 200.0, 120.0))
    good = KO.row_like(labels[0], 0.8, xyz=(-19.9, 1.5, 20.0))
    res = both([[low, good]], [labels])
    for metric in ('bev', '3d'):
        e = res[(metric, 'moderate')]
        # pass 1 takes the higher score -- the low detection: no true positive at all; the label stays a false negative of the dataset
        assert len(e['thresholds']) == 0
    # with the low detection's score below, pass 1 takes the good one (0.8); a second label's detection adds the threshold 0.4, at which
    # the low one is in again, comes first in row order, is taken as an ignored candidate (c) and displaced by the good one (b)
    labels = spread_labels(2)
    low = KO.row_like(labels[0], 0.5, box=(100.0, 100.0, 200.0, 120.0))
    good = KO.row_like(labels[0], 0.8, xyz=(-19.9, 1.5, 20.0))
    res = both([[low, good, KO.row_like(labels[1], 0.4)]], [labels])
    for metric in ('bev', '3d'):
        e = res[(metric, 'moderate')]
        assert (list(e['tp']), list(e['fp']), list(e['fn'])) == ([1, 2], [0, 0], [1, 0])


def test_ix_pass_1_takes_the_highest_score_and_pass_2_the_highest_overlap():
    labels = spread_labels(1)
    loose = KO.row_like(labels[0], 0.9, box=(104.0, 100.0, 204.0, 160.0), xyz=(-19.7, 1.5, 20.0))
    tight = KO.row_like(labels[0], 0.6)
    res = both([[loose, tight]], [labels])
    for metric in METRICS:
        e = res[(metric, 'easy')]
        # pass 1: the true positive is the one of score 0.9, the only threshold; pass 2 at 0.9 sees the loose one alone
        assert [float(t) for t in e['thresholds']] == [float(np.float32(0.9))]
        assert (list(e['tp']), list(e['fp']), list(e['fn'])) == ([1], [0], [0])
    # three labels, so that a second threshold (0.6, from another label's detection) lets both in: the tight one is the tp, the loose one an fp
    labels = spread_labels(3)
    loose = KO.row_like(labels[0], 0.9, box=(104.0, 100.0, 204.0, 160.0), xyz=(-19.7, 1.5, 20.0))
    tight = KO.row_like(labels[0], 0.7)
    other = KO.row_like(labels[1], 0.6)
    res = both([[loose, tight, other]], [labels])
    for metric in METRICS:
        e = res[(metric, 'easy')]
        assert [float(t) for t in e['thresholds']] == [float(np.float32(0.9)), float(np.float32(0.6))]
        assert (list(e['tp']), list(e['fp']), list(e['fn'])) == ([1, 2], [0, 1], [2, 1])


def test_x_equal_scores_keep_the_first():
    labels = spread_labels(1)
    first = KO.row_like(labels[0], 0.8, alpha=0.0)
    second = KO.row_like(labels[0], 0.8, alpha=math.pi)             # the same box: had it won, the similarity would be 0
    res = both([[first, second]], [labels])
    assert (list(res[('image', 'easy')]['tp']), list(res[('image', 'easy')]['fp'])) == ([1], [1])
    assert res[('aos', 'easy')]['aos_r11'] == pytest.approx(100.0 * 0.5 / 11.0, abs=1e-9)    # one recall point: similarity 1 over tp + fp = 2
    one = KO.match(np.array([first, second]), np.array(labels), KO.image_overlaps([first, second], labels), 0, 0, 0.7)
    assert one['tp'] == 1 and one['tp_scores'][0] == np.float32(0.8)


def test_xi_aos_is_ap_with_exact_alphas_and_half_of_it_a_quarter_turn_off():
    labels = spread_labels(4, alpha=0.3)
    rows = [KO.row_like(g, 0.9 - 0.1 * k) for k, g in enumerate(labels)] + [KO.make_row(0.85, box=(800.0, 300.0, 900.0, 360.0), xyz=(15.0, 1.5, 50.0))]
    res = both([rows], [labels])
    for diff in DIFFS:
        assert res[('aos', diff)]['aos_r40'] == pytest.approx(res[('image', diff)]['ap_r40'], abs=1e-9)
        assert 0 < res[('image', diff)]['ap_r40'] < 100
    turned = [r.copy() for r in rows]
    for r in turned:
        r[25] = np.float32(0.3 + math.pi / 2)
    res = both([turned], [labels])
    for diff in DIFFS:
        assert res[('aos', diff)]['aos_r40'] == pytest.approx(res[('image', diff)]['ap_r40'] / 2, abs=1e-5)      # (float32 alpha)
        assert res[('aos', diff)]['aos_r11'] == pytest.approx(res[('image', diff)]['ap_r11'] / 2, abs=1e-5)


def test_a_random_dataset_agrees_with_the_oracle():
    rng = np.random.default_rng(22)
    scenes = [KO.random_scene(rng, int(rng.integers(1, 9)), int(rng.integers(0, 30))) for _ in range(6)]
    scenes.append((np.zeros((0, 36), np.float32), scenes[0][1]))
    scenes.append((scenes[1][0], np.zeros((0, 16))))
    res = both([s[0] for s in scenes], [s[1] for s in scenes])
    assert sum(int(res[(m, 'hard')]['tp'][-1]) for m in METRICS if len(res[(m, 'hard')]['tp'])) > 0


def test_min_overlap_is_an_argument():
    row, label = exact_pair(5)                                # IoU 5/15
    assert list(both([[row]], [[label]], (0.3, 0.3, 0.3))[('3d', 'easy')]['tp']) == [1]
    assert len(both([[row]], [[label]], (0.3, 0.5, 0.3))[('bev', 'easy')]['thresholds']) == 0
    with pytest.raises(ValueError):
        kitti_eval.evaluate_rows([[row]], [[label]], (0.7, 0.7))


# ---------------------------------------------------------------------------------------------------- files and the command line
LABEL_TEXT = ('Car 0.00 0 -1.58 587.01 173.33 614.12 200.12 1.65 1.67 3.64 -0.65 1.71 46.70 -1.59\n'
              'Van 0.10 1 1.20 100.00 150.00 220.00 260.00 2.10 1.90 5.20 -8.00 1.80 20.00 1.10\n'
              'Cyclist 0.00 0 -2.46 665.45 160.00 717.93 217.99 1.72 0.47 1.65 2.45 1.35 22.10 -2.35\n'
              'DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10\n')


write_dataset = KO.write_dataset


def test_parsing_of_label_and_result_files(tmp_path):
    path = tmp_path / 'label.txt'
    path.write_text(LABEL_TEXT)
    labels = kitti_eval.read_label_file(str(path))
    assert labels.shape == (4, 16) and labels[:, 0].tolist() == [0, 1, 3, 2] and (labels[:, 15] == 0).all()
    assert labels[0, 1:15].tolist() == [0.0, 0, -1.58, 587.01, 173.33, 614.12, 200.12, 1.65, 1.67, 3.64, -0.65, 1.71, 46.70, -1.59]
    as_result = kitti_eval.read_result_file(str(path))                       # 15 fields: the score is 1
    assert (as_result[:, 15] == 1.0).all()
    rows = kitti_eval.rows_from_results(as_result, D=3)                      # the Car only; padding rows are -1
    assert (rows[1:] == -1).all() and rows[0, 14] == 0 and rows[0, 12] == 1
    assert rows[0, [25, 26, 27, 28, 29, 30, 17, 18, 19, 31, 21, 32]].tolist() == np.array(labels[0, 3:15], np.float32).tolist()
    # what kitti_lines_from_rows writes comes back as the same rows, to the two decimals of the text
    rng = np.random.default_rng(24)
    src, _ = KO.random_scene(rng, 4, 7)
    out = tmp_path / 'result.txt'
    out.write_text(gpp_utils.kitti_lines_from_rows(src, 7))
    back = kitti_eval.rows_from_results(kitti_eval.read_result_file(str(out)))
    cols = list(gpp_utils.KITTI_COLUMNS)
    assert back.shape == (7, 36) and np.abs(back[:, cols] - src[:, cols]).max() <= 0.005 + 1e-4
    with pytest.raises(ValueError):
        bad = tmp_path / 'bad.txt'
        bad.write_text('Car 0 0 0\n')
        kitti_eval.read_label_file(str(bad))


def test_evaluate_kitti_on_files_agrees_with_the_oracle_and_with_rows(tmp_path):
    label_dir, result_dir = write_dataset(tmp_path)
    res = kitti_eval.evaluate_kitti(label_dir, result_dir)
    names = sorted(os.listdir(label_dir))
    labels = [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in names]
    rows = [kitti_eval.rows_from_results(kitti_eval.read_result_file(os.path.join(result_dir, f))) for f in names]
    want = both(rows, labels)
    by_rows = kitti_eval.evaluate_kitti(label_dir, rows={f[:-4]: r for f, r in zip(names, rows)})
    for key in want:
        for name, value in want[key].items():
            assert np.array_equal(res[key][name], value, equal_nan=True) and np.array_equal(by_rows[key][name], value, equal_nan=True), (key, name)
    with pytest.raises(ValueError):
        kitti_eval.evaluate_kitti(label_dir)


def test_the_command_line_scores_a_directory(tmp_path, capsys):
    from keras_retinanet_3D.bin import evaluate_kitti as cli
    label_dir, result_dir = write_dataset(tmp_path)
    out = str(tmp_path / 'scores.json')
    res = cli.main([label_dir, result_dir, '--json', out])
    text = capsys.readouterr().out
    assert 'Car bbox AP' in text and 'Car bev  AP' in text and 'Car 3d   AP' in text and 'Car aos' in text
    stored = json.load(open(out))
    assert len(stored) == 12
    for (a, b), entry in res.items():
        for name, value in entry.items():
            assert np.array_equal(np.asarray(stored['{}_{}'.format(a, b)][name], dtype=np.asarray(value).dtype), value, equal_nan=True)
    with pytest.raises(SystemExit):
        cli.main([label_dir])


# ---------------------------------------------------------------------------------------------------- refusals, on the host
def test_the_entry_points_check_their_arguments_before_any_launch():
    lib = hip.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    mo = (ctypes.c_double * 3)(0.7, 0.7, 0.7)

    def overlaps(ptrs=None, B=2, D=100, A=4):
        ptrs = [p] * 4 if ptrs is None else ptrs
        return lib.gpp_kitti_overlaps_f64(ptrs[0], ptrs[1], ptrs[2], B, D, A, ptrs[3], None)

    for k in range(4):
        assert overlaps([None if j == k else p for j in range(4)]) == -1, k
    for kw in ({'B': -1}, {'D': -1}, {'A': -1}):
        assert overlaps(**kw) == -1, kw
    assert overlaps(B=0) == 0 and overlaps(D=0) == 0 and overlaps(B=0, ptrs=[None] * 4) == 0
    assert overlaps(D=129) == -4 and overlaps(A=129) == -4

    def stats(ptrs=None, min_overlap=mo, B=2, D=100, A=4, T=41, second=True):
        # rows labels counts overlaps | thresholds n_thresholds | tp_scores n_gt stats similarity
        ptrs = [p] * 10 if ptrs is None else list(ptrs)
        if not second:
            ptrs[4] = None
        return lib.gpp_kitti_stats_f64(ptrs[0], ptrs[1], ptrs[2], ptrs[3], min_overlap, ptrs[4], ptrs[5], B, D, A, T, ptrs[6], ptrs[7], ptrs[8], ptrs[9], None)

    for k in (0, 1, 2, 3, 5, 8, 9):                                # pass 2 needs these
        assert stats([None if j == k else p for j in range(10)]) == -1, k
    for k in (0, 1, 2, 3, 6, 7):                                   # pass 1 (no thresholds) needs these
        assert stats([None if j == k else p for j in range(10)], second=False) == -1, k
    assert stats(min_overlap=None) == -1
    for kw in ({'B': -1}, {'D': -1}, {'A': -1}, {'T': -1}, {'T': 42}):
        assert stats(**kw) == -1, kw
    assert stats(B=0) == 0 and stats(D=0) == 0 and stats(B=0, ptrs=[None] * 10) == 0
    assert stats(D=129) == -4 and stats(A=129) == -4 and stats(D=129, second=False) == -4
    assert (hip.GPP_KITTI_MAX_DETECTIONS, hip.GPP_KITTI_MAX_LABELS, hip.GPP_KITTI_MAX_THRESHOLDS) == (128, 128, 41)


def test_the_device_form_refuses_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    label_dir, result_dir = write_dataset(tmp_path, n=1)
    with pytest.raises(ValueError, match='HIP device'):
        kitti_eval.evaluate_kitti(label_dir, result_dir, device=True)
    from keras_retinanet_3D.bin import evaluate_kitti as cli
    with pytest.raises(ValueError, match='HIP device'):
        cli.main([label_dir, result_dir, '--device'])


def test_pipeline_and_sharded_model_refuse():
    from keras_retinanet_3D.utils.distributed import ShardedModel
    from keras_retinanet_3D.utils.pipeline import FramePipeline
    with pytest.raises(ValueError, match='score_poses_on_frames'):
        ShardedModel(object()).score_poses_on_frames(None, None, None, None)
    with pytest.raises(ValueError, match='score_poses_on_frames'):
        FramePipeline.score_poses_on_frames(None, None, None, None, None)
