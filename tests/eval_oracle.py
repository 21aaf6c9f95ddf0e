"""
ORACLE of the device matching (csrc/eval.hip, include/gpp.h gpp_eval_match_f32): the rules of utils/eval.py's
_image_rows + _match_bin (reference utils/eval.py:93-118, :207-226) written as loops over one detection and one annotation at a time,
with Python floats (IEEE float64, every operation separate) and the reference's own serial form of the hit rule -- detections walk
in the stable descending order of their scores and take an annotation that is still free -- where the kernel takes a minimum over
ranks.  Nothing of utils.eval or utils.anchors is called here.
"""
import os
import sys

import numpy as np

ANN_COLS, ERR_COLS = 17, 11
EPS = sys.float_info.epsilon


def iou(a, b):
    """ utils/anchors.compute_overlap for one pair of boxes (4 Python floats each), operation for operation """
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    iw = iw if iw > 0.0 else 0.0
    ih = ih if ih > 0.0 else 0.0
    inter = iw * ih
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    union = area_a + area_b - inter
    union = union if union > EPS else EPS
    return inter / union


def bin_of(label, orientation, num_classes):
    """ 4 * label + orientation for an integer-valued pair in range, else -1 (the host compares with the integers of its two loops) """
    if label != int(label) or orientation != int(orientation):
        return -1
    label, orientation = int(label), int(orientation)
    return 4 * label + orientation if 0 <= label < num_classes and 0 <= orientation < 4 else -1


def match(outputs, scales, annotations, num_classes, score_threshold=0.05, max_detections=100, iou_threshold=0.5):
    """ outputs: the first five model outputs (boxes (B, D, 12), dimensions (B, D, 3), scores (B, D) float32, labels, orientations
    (B, D) int32); scales: one per image; annotations: per image an (n, 17) float64 array.
    -> table (B, D, 3) int32, errors (B, D, 11) float64, counts (B,) int32 """
    boxes, dims, scores, labels, orientations = [np.asarray(o) for o in outputs[:5]]
    B, D = scores.shape
    table = np.full((B, D, 3), -1, np.int32)
    errors = np.zeros((B, D, ERR_COLS), np.float64)
    counts = np.zeros((B,), np.int32)
    thr = np.float32(score_threshold)
    for b in range(B):
        ann = np.asarray(annotations[b], np.float64).reshape(-1, ANN_COLS)
        scale = np.float32(scales[b])
        # the stable descending order: a higher score first, of two equal scores the lower index
        kept = [d for d in range(D) if scores[b, d] > thr]
        order = sorted(kept, key=lambda d: (-float(scores[b, d]), d))[:max_detections]
        counts[b] = len(order)
        taken = set()
        for d in order:
            label = bin_of(labels[b, d], orientations[b, d], num_classes)
            table[b, d] = label, 0, -1
            if label < 0:
                continue
            pixels = [float(np.float32(v) / scale) for v in boxes[b, d]]          # float32 / float32, then widened
            best, claim = -1.0, -1
            for a in range(ann.shape[0]):
                if bin_of(ann[a, 15], ann[a, 16], num_classes) != label:
                    continue
                v = iou(pixels[:4], [float(x) for x in ann[a, :4]])
                if v > best:                                                      # the FIRST maximum
                    best, claim = v, a
            table[b, d, 2] = claim
            if claim >= 0 and best >= iou_threshold and claim not in taken:
                taken.add(claim)
                table[b, d, 1] = 1
                mine = pixels[4:12] + [float(v) for v in dims[b, d]]
                errors[b, d] = [abs(mine[k] - float(ann[claim, 4 + k])) for k in range(ERR_COLS)]
    return table, errors, counts


# ---------------------------------------------------------------------------------------------------- the committed goldens
GOLDENS = ('eval_small', 'eval_ties', 'eval_two_classes')
SETTINGS = {'default': {'iou_threshold': 0.5, 'score_threshold': 0.05, 'max_detections': 100},
            'strict': {'iou_threshold': 0.7, 'score_threshold': 0.3, 'max_detections': 5}}          # tests/test_eval.py SETTINGS, defaults spelt out


def load_golden(name):
    """ (golden dict, the first five outputs, scales, per-image annotation arrays, num_classes) of tests/golden/<name>.npz """
    import helpers
    g = dict(np.load(os.path.join(helpers.GOLDEN, name + '.npz')))
    annotations = np.split(g['annotations'], np.cumsum(g['ann_counts'])[:-1], axis=0)
    return g, [g['outputs_{}'.format(j)] for j in range(5)], g['scales'], annotations, int(g['num_classes'])


def bins_of_annotations(annotations, num_classes):
    """ all_annotations[image][bin] as utils.eval._get_annotations lays them out, from per-image (n, 17) arrays """
    return [[a[np.logical_and(a[:, 15] == label, a[:, 16] == orientation), :15] for label in range(num_classes) for orientation in range(4)]
            for a in annotations]


def assert_meets_golden(results, g, tag):
    """ the bar of tests/test_eval.py::test_evaluate_matches_the_reference """
    aps, ke, he, we, le = results
    want = g[tag + '_ap']
    assert sorted(aps) == list(range(len(want)))
    for label in aps:
        assert abs(float(aps[label][0]) - want[label, 0]) < 1e-12 and float(aps[label][1]) == want[label, 1], (label, aps[label], want[label])
    assert np.allclose([ke, he, we, le], g[tag + '_errors'], rtol=0, atol=1e-12)
