""" The device form of the evaluation on the GPU (csrc/eval.hip): gpp_eval_match_f32 against the loop-written oracle
(tests/eval_oracle.py) on the reference's goldens and on seeded cases built around its rules -- exact: table, counts, and the errors
byte for byte --, then through the model: the tensor-level helper against the host's _match_bin on the fetched outputs, and
evaluate(device=True) against evaluate() on a directory of frames of the four KITTI sizes. """
import os

import numpy as np
import pytest
import torch

import eval_oracle
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.preprocessing import kitti
from keras_retinanet_3D.utils import eval as gpp_eval
from keras_retinanet_3D.utils import image as I
from keras_retinanet_3D.utils import synthetic

pytestmark = pytest.mark.gpu


def device_match(outputs, scales, annotations, num_classes, score_threshold=0.05, max_detections=100, iou_threshold=0.5):
    """ gpp_eval_match_f32 through its binding on host arrays -> (table, errors, counts) as NumPy.  The padding rows of the annotation
    table hold a box that covers everything, in bin 0: a kernel that read past an image's count would show it. """
    dev = torch.device('cuda')
    B = len(annotations)
    padded = np.zeros((B, max(len(a) for a in annotations), 17))
    padded[:, :, :4] = -1e6, -1e6, 1e6, 1e6
    for b, a in enumerate(annotations):
        padded[b, :len(a)] = a
    put = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    table, errors, counts = hip.eval_match(*([put(o) for o in outputs[:5]] + [
        put(np.asarray(scales, np.float64).astype(np.float32)), put(padded), put(np.asarray([len(a) for a in annotations], np.int32)),
        num_classes, score_threshold, max_detections, iou_threshold]))
    torch.cuda.synchronize()
    return table.cpu().numpy(), errors.cpu().numpy(), counts.cpu().numpy()


def assert_is_the_oracles(got, want):
    for name, g, w in zip(('table', 'errors', 'counts'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if not np.array_equal(g, w):
            where = np.argwhere(g != w)[:5]
            raise AssertionError('{} differs at {}: {} != {}'.format(name, where.tolist(), g[tuple(where[0])], w[tuple(where[0])]))
    assert got[1].tobytes() == want[1].tobytes()


# ---------------------------------------------------------------------------------------------------- (a) the reference's goldens
@pytest.mark.parametrize('tag', sorted(eval_oracle.SETTINGS))
@pytest.mark.parametrize('name', eval_oracle.GOLDENS)
def test_goldens_through_the_kernel(name, tag):
    g, outputs, scales, annotations, num_classes = eval_oracle.load_golden(name)
    got = device_match(outputs, scales, annotations, num_classes, **eval_oracle.SETTINGS[tag])
    assert_is_the_oracles(got, eval_oracle.match(outputs, scales, annotations, num_classes, **eval_oracle.SETTINGS[tag]))
    assert int((got[0][:, :, 1] == 1).sum()) > 0
    results = gpp_eval.assemble_matches(list(got[0]), list(outputs[2]), list(got[1]), eval_oracle.bins_of_annotations(annotations, num_classes), num_classes)
    eval_oracle.assert_meets_golden(results, g, tag)


# ---------------------------------------------------------------------------------------------------- (b) seeded cases
B = 3
SCALES = [1.0, 1333.0 / 1242.0, 0.75]


def base_case(seed, D, A, num_classes=1, copies=3):
    """ per image A annotations spread over the bins and D rows: `copies` jittered copies of every annotation that fits (several
    detections around one annotation, in its bin), free boxes, and a tail of padding rows (-1).  Scores are distinct. """
    rng = np.random.default_rng(seed)
    annotations, out = [], [np.full((B, D, 12), -1, np.float32), np.full((B, D, 3), -1, np.float32), np.full((B, D), -1, np.float32),
                            np.full((B, D), -1, np.int32), np.full((B, D), -1, np.int32)]
    live = D - D // 10
    for b in range(B):
        ann = np.zeros((A, 17))
        ann[:, :2] = rng.uniform(0, 900, (A, 2))
        ann[:, 2:4] = ann[:, :2] + rng.uniform(20, 200, (A, 2))
        ann[:, 4:12] = rng.uniform(0, 1200, (A, 8))
        ann[:, 12:15] = rng.uniform(1, 5, (A, 3))
        ann[:, 15] = rng.integers(0, num_classes, A)
        ann[:, 16] = rng.integers(0, 4, A)
        annotations.append(ann)
        boxes = np.zeros((live, 12))
        boxes[:, :2] = rng.uniform(0, 900, (live, 2))
        boxes[:, 2:4] = boxes[:, :2] + rng.uniform(20, 200, (live, 2))
        boxes[:, 4:] = rng.uniform(0, 1200, (live, 8))
        labels, orient = rng.integers(0, num_classes, live), rng.integers(0, 4, live)
        near = min(copies * A, 2 * live // 3)
        for d in range(near):
            a = d % A
            boxes[d, :4] = ann[a, :4] + rng.uniform(-0.12, 0.12, 4) * np.tile(ann[a, 2:4] - ann[a, :2], 2)
            boxes[d, 4:] = ann[a, 4:12] + rng.uniform(-3, 3, 8)
            labels[d], orient[d] = ann[a, 15], ann[a, 16]
        out[0][b, :live] = boxes * SCALES[b]
        out[1][b, :live] = rng.uniform(1, 5, (live, 3))
        out[2][b, :live] = rng.permutation(np.linspace(0.06, 0.99, live)).astype(np.float32)
        out[3][b, :live], out[4][b, :live] = labels, orient
    return out, annotations


def case_large():
    return base_case(1, 300, 70), {}


def case_shuffled():
    (out, ann), _ = case_large()
    perm = np.random.default_rng(2).permutation(300)
    return ([o[:, perm] for o in out], ann), {}


def case_duplicate_annotations():
    out, ann = base_case(3, 40, 9)
    for b in range(B):
        ann[b][4] = ann[b][1]                                     # two annotations, one box, one bin: the first is claimed ...
        ann[b][4, 4:15] += 7.0                                    # (... and the errors say which)
        out[0][b, 1, :4] = (ann[b][1, :4] * SCALES[b]).astype(np.float32)          # ... by two detections on that box: the second finds
        out[0][b, 10, :4] = out[0][b, 1, :4]                      # it taken, though its twin is free
        out[3][b, [1, 10]], out[4][b, [1, 10]] = ann[b][1, 15], ann[b][1, 16]
        out[2][b, 1] = np.float32(0.995)
    return (out, ann), {}


def case_crowded():
    out, ann = base_case(4, 60, 4, copies=9)                      # 9 detections around each of 4 annotations ...
    for b in range(B):
        out[2][b, :8] = np.float32(0.97)                          # ... the best eight with one score: the lower index goes first
    return (out, ann), {}


def case_iou_at_the_threshold():
    out, ann = base_case(5, 40, 9)
    for b in range(B):
        ann[b][0, :4] = 0.0, 0.0, 2.0, 2.0
        ann[b][0, 15:] = 0, 0
        out[0][b, 0, :4] = np.array([1.0, 0.0, 3.0, 2.0], np.float32) * np.float32(1.0 if b == 0 else 2.0)
        out[3][b, 0], out[4][b, 0], out[2][b, 0] = 0, 0, np.float32(0.995)
    scales = [1.0, 2.0, 2.0]
    thr = eval_oracle.iou([1.0, 0.0, 3.0, 2.0], [0.0, 0.0, 2.0, 2.0])          # 2 / 6 in float64: >= itself is a hit
    return (out, ann), {'iou_threshold': thr, 'scales': scales, 'hit': (0, 0)}


def case_iou_just_below_the_threshold():
    (out, ann), kw = case_iou_at_the_threshold()
    return (out, ann), dict(kw, iou_threshold=float(np.nextafter(kw['iou_threshold'], 1.0)), hit=None, miss=(0, 0))


def case_score_at_the_threshold():
    out, ann = base_case(6, 40, 9)
    for b in range(B):
        out[2][b, :3] = np.float32(0.3)                           # float32(0.3) > float32(0.3) is false
    return (out, ann), {'score_threshold': 0.3, 'unselected': (0, 0)}


def case_max_detections():
    return base_case(7, 40, 9), {'max_detections': 7}


def case_zero_area():
    out, ann = base_case(8, 40, 9)
    for b in range(B):
        out[0][b, 0, 2] = out[0][b, 0, 0]                         # a detection without width
        out[0][b, 1, 2:4] = out[0][b, 1, :2]                      # a point
        ann[b][2, 2:4] = ann[b][2, :2]                            # an annotation that is a point ...
        out[0][b, 2, :4] = np.tile(ann[b][2, :2], 2).astype(np.float32)          # ... and a detection on it: 0 / eps
        out[3][b, 2], out[4][b, 2] = ann[b][2, 15], ann[b][2, 16]
    return (out, ann), {'scales': [1.0, 1.0, 1.0]}


def case_image_without_annotations():
    out, ann = base_case(9, 40, 9)
    ann[1] = np.zeros((0, 17))
    return (out, ann), {}


def case_image_without_detections():
    out, ann = base_case(10, 40, 9)
    out[2][2] = np.minimum(out[2][2], np.float32(0.05))
    return (out, ann), {}


def case_two_classes():
    out, ann = base_case(11, 60, 12, num_classes=2)
    for b in range(B):
        out[3][b, 5] = 2                                          # a label beyond the classes, an orientation beyond 3: selected, in no bin
        out[4][b, 6] = 4
    return (out, ann), {'num_classes': 2}


CASES = [case_large, case_shuffled, case_duplicate_annotations, case_crowded, case_iou_at_the_threshold, case_iou_just_below_the_threshold,
         case_score_at_the_threshold, case_max_detections, case_zero_area, case_image_without_annotations, case_image_without_detections,
         case_two_classes]


@pytest.mark.parametrize('case', CASES, ids=[c.__name__[5:] for c in CASES])
def test_seeded_cases_against_the_oracle(case):
    (out, ann), kw = case()
    kw = dict(kw)
    scales, hit, miss, unselected = kw.pop('scales', SCALES), kw.pop('hit', None), kw.pop('miss', None), kw.pop('unselected', None)
    num_classes = kw.pop('num_classes', 1)
    want = eval_oracle.match(out, scales, ann, num_classes, **kw)
    # the case holds what its name says
    assert int((want[0][:, :, 1] == 1).sum()) > 0 and int((want[0][:, :, 1] == 0).sum()) > 0
    if hit is not None:
        assert want[0][hit][1] == 1
    if miss is not None:
        assert tuple(want[0][miss][1:]) == (0, 0)
    if unselected is not None:
        assert tuple(want[0][unselected]) == (-1, -1, -1)
    if case is case_max_detections:
        assert want[2].tolist() == [7] * B
    if case is case_image_without_annotations:
        assert (want[0][1, :, 2] == -1).all() and want[2][1] > 0
    if case is case_image_without_detections:
        assert want[2][2] == 0 and want[2][0] > 0
    if case is case_duplicate_annotations:
        assert want[0][:, 1].tolist() != want[0][:, 10].tolist() and (want[0][:, [1, 10], 2] == 1).all()
    if case is case_two_classes:
        assert set(np.unique(want[0][:, :, 0])) >= {-1, 0, 7} and tuple(want[0][0, 5]) == (-1, 0, -1)
    got = device_match(out, scales, ann, num_classes, **kw)
    assert_is_the_oracles(got, want)
    if case is case_shuffled:                                     # distinct scores: the table moves with its detections
        (plain, _), _ = case_large()
        perm = np.random.default_rng(2).permutation(300)
        first = device_match(plain, scales, ann, num_classes)
        assert np.array_equal(first[0][:, perm], got[0]) and first[1][:, perm].tobytes() == got[1].tobytes() and np.array_equal(first[2], got[2])


def test_limits_of_the_kernel():
    """ D = A = 1024, the largest supported image, against the oracle on one image (B = 1: the oracle is a Python loop) """
    rng = np.random.default_rng(12)
    (out, ann), _ = case_large()
    D, A = hip.GPP_EVAL_MAX_DETECTIONS, hip.GPP_EVAL_MAX_ANNOTATIONS
    pick_d, pick_a = rng.integers(0, 270, D), rng.integers(0, 70, A)
    one = [np.ascontiguousarray(o[:1, pick_d]) for o in out]
    one[2][0] = rng.permutation(np.linspace(0.0, 1.0, D)).astype(np.float32)
    anns = [ann[0][pick_a]]
    kw = {'score_threshold': 0.9, 'max_detections': 64, 'iou_threshold': 0.5}
    assert_is_the_oracles(device_match(one, [SCALES[0]], anns, 1, **kw), eval_oracle.match(one, [SCALES[0]], anns, 1, **kw))


# ---------------------------------------------------------------------------------------------------- (c), (d): through the model
def labels_from_rows(rows):
    """ annotations (n, 17) made from the host path's own detection rows of one image (utils.eval._image_rows): by turns a copy, a
    copy shifted by a fifth of its width (IoU 2/3), one shifted by half (IoU 1/3), and a copy in the next orientation bin """
    out = []
    for j, r in enumerate(rows[:16]):
        box, rest, label, orientation = r[:4].copy(), r[4:15].copy(), r[-1], r[-2]
        if j % 4 in (1, 2):
            box[[0, 2]] += (0.2 if j % 4 == 1 else 0.5) * (box[2] - box[0])
            rest += 1.5
        if j % 4 == 3:
            orientation = (orientation + 1) % 4
        out.append(np.concatenate([box, rest, [label, orientation]]))
    return np.asarray(out, np.float64).reshape(-1, 17)


def test_the_tensor_level_helper_equals_the_hosts_matching(monkeypatch):
    """ resnet50 f32 on four small images: match_outputs on the plan's device outputs against _match_bin on the fetched ones """
    from test_eval import GoldenGenerator, GoldenModel
    from test_ragged_gpu import small_batch
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    model = models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype='f32')
    images, P_inv, planes = small_batch(5)
    outputs = model.predict_on_batch([images, P_inv, planes])
    plan = model._last_plan
    scales = [1.0, 1333.0 / 1242.0, 0.8, 2.0]
    annotations = [labels_from_rows(gpp_eval._image_rows(outputs, k, scales[k], 0.05, 100)) for k in range(4)]
    assert sum(len(a) for a in annotations) > 0
    # (synthetic weights score around 0.06: the second setting cuts inside that range, where the goldens' strict setting would keep nothing)
    for settings in (eval_oracle.SETTINGS['default'], {'iou_threshold': 0.7, 'score_threshold': 0.055, 'max_detections': 5}):
        table, scores, errors, counts = model.match_outputs(model.outputs(plan), scales, annotations, num_classes=1, **settings)
        assert np.array_equal(scores, outputs[2])
        hits_seen = 0
        for k in range(4):
            rows = gpp_eval._image_rows(outputs, k, scales[k], settings['score_threshold'], settings['max_detections'])
            assert counts[k] == len(rows)
            order = np.flatnonzero(table[k, :, 1] >= 0)
            order = order[np.argsort(-scores[k, order], kind='stable')]
            for label in range(4):
                mine = rows[np.logical_and(rows[:, -1] == 0, rows[:, -2] == label)]
                theirs = annotations[k][annotations[k][:, 16] == label, :15]
                hits, errs = gpp_eval._match_bin(mine[:, :-2], theirs, settings['iou_threshold'])
                pick = order[table[k, order, 0] == label]
                assert np.array_equal(table[k, pick, 1] == 1, hits), (k, label)
                assert np.array_equal(errors[k, pick[hits]], np.asarray(errs).reshape(-1, 11)), (k, label)
                hits_seen += int(hits.sum())
        assert hits_seen > 0
        # the results: evaluate() replaying the fetched outputs
        g = {'planes': planes[0], 'scales': np.asarray(scales), 'num_classes': 1, 'annotations': np.concatenate(annotations),
             'ann_counts': np.asarray([len(a) for a in annotations])}
        g.update({'outputs_{}'.format(j): o for j, o in enumerate(outputs)})
        want = gpp_eval.evaluate(GoldenGenerator(g), GoldenModel(g), batch_size=4, **settings)
        got = gpp_eval.assemble_matches(list(table), list(scores), list(errors), eval_oracle.bins_of_annotations(annotations, 1), 1)
        assert got == want


def test_evaluate_on_the_device_returns_what_the_host_path_returns(tmp_path, monkeypatch):
    """ a directory of four PNG frames, one of each KITTI size, with labels made from the model's own detections, read by KittiGenerator:
    evaluate(device=True, batch_size=4) == evaluate(batch_size=4), resnet50 f16x3 """
    import scipy.io
    from PIL import Image
    from test_ragged_gpu import KITTI_SHAPES
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    model = models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype='f16x3')
    frames = [(np.random.default_rng(40 + i).integers(0, 2, size=s + (3,)) * 255).astype(np.uint8) for i, s in enumerate(KITTI_SHAPES)]
    planes = synthetic.load_plane_database('100')
    P2 = synthetic.KITTI_LIKE_P2
    P_inv = np.stack([synthetic.synthetic_calibration(I.compute_resize_scale(f.shape))[1] for f in frames])
    outputs, scales = model.predict_on_frames(frames, P_inv, np.tile(planes[None], (4, 1, 1)))
    for d in ('images', 'labels', 'calibs'):
        os.makedirs(str(tmp_path / 'val' / d))
    scipy.io.savemat(str(tmp_path / 'road_planes_database.mat'), {'road_planes_database': planes})
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    n_labels = 0
    for k, f in enumerate(frames):
        Image.fromarray(f[:, :, ::-1]).save(str(tmp_path / 'val' / 'images' / ('%06d.png' % k)))
        (tmp_path / 'val' / 'calibs' / ('%06d.txt' % k)).write_text(calib)
        rows = labels_from_rows(gpp_eval._image_rows(outputs, k, float(scales[k]), 0.05, 100))
        n_labels += len(rows)
        (tmp_path / 'val' / 'labels' / ('%06d.txt' % k)).write_text(''.join(
            'Car 0 0 0 ' + ' '.join(repr(float(v)) for v in r[:15]) + ' %d\n' % int(r[16]) for r in rows))
    assert n_labels > 0
    gen = kitti.KittiGenerator(str(tmp_path), subset='val')
    assert gen.size() == 4 and sum(len(gen.load_annotations(i)[0]) for i in range(4)) == n_labels
    want = gpp_eval.evaluate(gen, model, batch_size=4)
    got = gpp_eval.evaluate(gen, model, batch_size=4, device=True)
    assert got == want
    assert len(model._plans) == 1                                 # one ragged plan served the labels, the host path and the device path
    assert sum(n for _, n in got[0].values()) == n_labels and max(ap for ap, _ in got[0].values()) > 0 and got[1] > 0
