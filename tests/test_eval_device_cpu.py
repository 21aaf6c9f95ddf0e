""" The device form of the evaluation without a GPU: the oracle of the matching (tests/eval_oracle.py) fed through
utils.eval.assemble_matches reproduces the reference's goldens, gpp_eval_match_f32 refuses bad arguments on the host before any launch
(as tests/test_ragged_cpu.py checks its entry points), and evaluate(device=True) says what a model has to offer. """
import ctypes

import numpy as np
import pytest

import eval_oracle
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import eval as gpp_eval


@pytest.mark.parametrize('tag', sorted(eval_oracle.SETTINGS))
@pytest.mark.parametrize('name', eval_oracle.GOLDENS)
def test_the_oracles_table_assembles_into_the_golden(name, tag):
    g, outputs, scales, annotations, num_classes = eval_oracle.load_golden(name)
    table, errors, counts = eval_oracle.match(outputs, scales, annotations, num_classes, **eval_oracle.SETTINGS[tag])
    assert np.array_equal(counts, (table[:, :, 1] >= 0).sum(axis=1))
    results = gpp_eval.assemble_matches(list(table), list(outputs[2]), list(errors), eval_oracle.bins_of_annotations(annotations, num_classes), num_classes)
    eval_oracle.assert_meets_golden(results, g, tag)
    # the oracle selects what the reference selected: per (image, bin) the golden's detection counts
    per_bin = np.array([[(t[:, 0] == label).sum() for label in range(4 * num_classes)] for t in table])
    assert np.array_equal(per_bin, g[tag + '_det_counts'])


def test_assembly_keeps_the_host_order_and_ignores_unselected_rows():
    # one image, one class: detection 2 (score 0.9) before 0 (0.5) before 3 (0.5: the same score, the higher index); 1 is not selected
    table = np.array([[0, 0, 0], [-1, -1, -1], [0, 1, 0], [1, 1, 1]], np.int32)
    scores = np.array([0.5, 0.7, 0.9, 0.5], np.float32)
    errors = np.zeros((4, 11))
    errors[2], errors[3] = 2.0, 4.0
    annotations = [[np.zeros((1, 15)), np.zeros((1, 15)), np.zeros((0, 15)), np.zeros((0, 15))]]
    aps, ke, he, we, le = gpp_eval.assemble_matches([table], [scores], [errors], annotations, 1)
    assert aps == {0: (1.0, 1.0), 1: (1.0, 1.0), 2: (0, 0), 3: (0, 0)}
    assert (ke, he, we, le) == (3.0, 3.0, 3.0, 3.0)


# ---------------------------------------------------------------------------------------------------- the C ABI, on the host
def test_the_entry_point_checks_its_arguments_before_any_launch():
    lib = hip.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(ptrs=None, B=2, D=100, A=4, num_classes=1, max_detections=100):
        ptrs = [p] * 11 if ptrs is None else ptrs
        return lib.gpp_eval_match_f32(*(ptrs[:8] + [B, D, A, num_classes, 0.05, max_detections, 0.5] + ptrs[8:] + [None]))

    for k in range(11):                                          # every pointer, inputs and outputs
        assert call([None if j == k else p for j in range(11)]) == -1, k
    for kw in ({'B': -1}, {'D': -1}, {'A': -1}, {'num_classes': -1}, {'max_detections': -1}):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0 and call(D=0) == 0                     # nothing to do: nothing launched
    assert call(B=0, ptrs=[None] * 11) == 0
    assert call(D=hip.GPP_EVAL_MAX_DETECTIONS + 1) == -4 and call(A=hip.GPP_EVAL_MAX_ANNOTATIONS + 1) == -4
    assert (hip.GPP_EVAL_MAX_DETECTIONS, hip.GPP_EVAL_MAX_ANNOTATIONS) >= (1024, 1024)


# ---------------------------------------------------------------------------------------------------- evaluate(device=True)
def test_a_model_without_the_method_is_refused():
    from test_eval import GoldenGenerator, GoldenModel
    g = eval_oracle.load_golden('eval_small')[0]
    with pytest.raises(ValueError, match='match_on_frames'):
        gpp_eval.evaluate(GoldenGenerator(g), GoldenModel(g), device=True)


def test_device_mode_feeds_raw_frames_and_never_calls_the_generators_preprocessing():
    """ evaluate(device=True) with a stand-in model whose match_on_frames answers with the oracle's table: uint8 frames, batches cut
    at a change of shape, P_inv of the scaled calibration, the golden's results """
    from test_eval import GoldenGenerator
    g, outputs, scales, annotations, num_classes = eval_oracle.load_golden('eval_small')

    class Generator(GoldenGenerator):
        def load_image(self, i):
            return np.zeros((4 + i // 4, 6, 3), np.uint8)      # images 0-3 of one shape, 4-5 of another

        def preprocess_image(self, image):
            raise AssertionError('not called in device mode')

        resize_image = preprocess_image

    class Model(object):
        calls = []

        def match_on_frames(self, frames, P_inv, planes, anns, iou_threshold, score_threshold, max_detections, num_classes, min_side, max_side):
            B, first = len(frames), sum(self.calls)
            self.calls.append(B)
            assert frames.dtype == np.uint8 and frames.ndim == 4 and P_inv.shape == (B, 4, 3) and planes.shape == (B, 10, 4)
            assert (min_side, max_side) == (800, 1333) and num_classes == int(g['num_classes'])
            for k in range(B):
                assert np.array_equal(anns[k], annotations[first + k])
            table, errors, counts = eval_oracle.match([o[first:first + B] for o in outputs], scales[first:first + B], anns, num_classes,
                                                      score_threshold, max_detections, iou_threshold)
            return (table, outputs[2][first:first + B], errors, counts), None

    results = gpp_eval.evaluate(Generator(g), Model(), device=True, batch_size=3)
    assert Model.calls == [3, 1, 2]
    eval_oracle.assert_meets_golden(results, g, 'default')
