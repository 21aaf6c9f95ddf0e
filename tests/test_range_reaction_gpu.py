"""
dtype='f16x3' must never return a clamped activation as a plausible wrong answer (round-4 review, weak #3).

The IEEE-half halves of the headline type end at +-65504; an epilogue that has to clamp a stored activation counts it
(gpp_x3_range_events).  The model READS that counter with the results every synchronous call fetches anyway (model.fetch,
FramePipeline._collect: the 8 bytes ride behind the packed detections, no extra synchronisation) and reacts (`on_range_event`):
'f32' (default) runs the call again on a float32 twin and returns the reference-precision result, 'raise' refuses, 'ignore' is the old
behaviour.

The weights that provoke it compute the SAME function as the seeded ones: bn2a_branch2a's (gamma, beta) x 2^17 and res2a_branch2b's
kernel x 2^-17 -- a ReLU commutes with a positive scale and powers of two are exact, so at float32 every tensor behind branch2b is
bit-identical to the unscaled network's, while the map between the two layers holds values beyond 65504.

The second half of the file puts every other synchronous call (match_on_frames, the pose rows, their KITTI overlaps, the composites, a
ragged list of images and of frames) under the same weights: they all answer through RetinaNet3D._answer, and each returns what a
dtype='f32' model of those weights returns for the call, byte for byte.
"""
import numpy as np
import pytest

import helpers
from oracle import decode_np, net_torch
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import ledger, synthetic

pytestmark = pytest.mark.gpu

B, H, Wd = 2, 96, 160
SCALE = np.float32(2.0 ** 17)


def scaled_weights():
    w = dict(W.synthetic_weights('resnet50', 1234))
    w['bn2a_branch2a/gamma'] = w['bn2a_branch2a/gamma'] * SCALE
    w['bn2a_branch2a/beta'] = w['bn2a_branch2a/beta'] * SCALE
    w['res2a_branch2b/kernel'] = w['res2a_branch2b/kernel'] / SCALE
    return w


def inputs():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return [img, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]


def same(a, b):
    return all(helpers.bits_equal(x, y) if x.dtype.kind == 'f' else np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 8


@pytest.fixture(scope='module')
def f32_of_the_base_weights():
    return models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())


def test_a_call_whose_activations_leave_the_half_range_returns_the_float32_result(f32_of_the_base_weights, oracle_lib):
    w = scaled_weights()
    model = models.load_model(w, backbone_name='resnet50', dtype='f16x3')                    # on_range_event='f32' is the default
    assert model.on_range_event == 'f32' and model.range_fallbacks == 0
    out = model.predict_on_batch(inputs())
    assert model.range_fallbacks == 1
    want = models.load_model(w, backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())
    assert same(out, want)                                    # byte for byte what dtype='f32' returns for these weights
    assert same(out, f32_of_the_base_weights)                 # ... which is what the unscaled network returns at float32 (exact scaling)
    assert int((out[2] > 0.05).sum()) > 0
    # and that is the float32 CPU oracle's answer: same detections, orientations, plane indices (as __graft_entry__.smoke() checks f32)
    from keras_retinanet_3D.utils import anchors as A
    f = net_torch.forward(W.synthetic_weights('resnet50', 1234), inputs()[0], 'resnet50', storage=None)
    det, aidx = decode_np.detect(f['classification_logits'], f['regression'], f['regression_dim'], A.anchors_for_image((H, Wd)))
    kp, kpl, res, idx = helpers.c_oracle_poll(oracle_lib, det[0], det[1], det[4], inputs()[1], inputs()[2])
    twin_plan = model._twin.plan_for(B, H, Wd, 100, True)
    led = ledger.parity_ledger(list(det) + [kp, kpl, res], aidx, idx, out, twin_plan.anchor_index.cpu().numpy(), twin_plan.best_index.cpu().numpy())
    assert led['set_differences'] == 0 and led['same_orientation'] == led['common'] and led['same_plane'] == led['common'] > 0, led
    assert led['max_keypoint_rel_dev'] <= 1e-4, led
    # every further call is watched too
    again = model.predict_on_batch(inputs())
    assert model.range_fallbacks == 2 and same(again, want)


def test_raise_and_ignore():
    w = scaled_weights()
    strict = models.load_model(w, backbone_name='resnet50', dtype='f16x3')
    strict.on_range_event = 'raise'
    with pytest.raises(hip.GppError, match='half range'):
        strict.predict_on_batch(inputs())
    loose = models.load_model(w, backbone_name='resnet50', dtype='f16x3')
    loose.on_range_event = 'ignore'
    loose.x3_range_events(reset=True)
    got = loose.predict_on_batch(inputs())                    # the clamped map goes through: a finite, wrong answer
    assert loose.x3_range_events() > 0 and loose.range_fallbacks == 0
    want = models.load_model(w, backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())
    assert not same(got, want)


def test_sane_weights_never_take_the_fallback_and_the_packed_fetch_equals_the_eight_copies(f32_of_the_base_weights):
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
    out = model.predict_on_batch(inputs())
    plan = model.plan_for(B, H, Wd, 100, True)
    separate = model.fetch(plan, packed=False)
    assert model.range_fallbacks == 0 and model._twin is None
    assert same(out, separate)
    for a, b in zip(out, separate):
        assert a.dtype == b.dtype and a.shape == b.shape and a.flags.writeable
    assert int((out[2] > 0.05).sum()) == int((f32_of_the_base_weights[2] > 0.05).sum())       # (parity of the type: tests/test_fullsize_*.py)


def test_frame_pipeline_reruns_an_affected_batch_at_float32():
    from keras_retinanet_3D.utils import image
    from keras_retinanet_3D.utils.pipeline import FramePipeline
    w = scaled_weights()
    planes = synthetic.load_plane_database('100').astype(np.float32)
    scale = image.compute_resize_scale((375, 1242, 3))
    _, P_inv = synthetic.synthetic_calibration(scale)
    P_inv = np.tile(P_inv[None].astype(np.float32), (1, 1, 1))
    batches = [((np.random.default_rng(k).integers(0, 2, size=(1, 375, 1242, 3)) * 255).astype(np.uint8), P_inv, planes) for k in range(3)]
    ref = models.load_model(w, backbone_name='resnet50', dtype='f32')
    want = [ref.predict_on_frames(*b)[0] for b in batches]
    model = models.load_model(w, backbone_name='resnet50', dtype='f16x3')
    got = list(FramePipeline(model, depth=3).run(iter(batches)))
    assert model.range_fallbacks == 3
    for (outs, _), r in zip(got, want):
        assert same(outs, r)


def test_a_sharded_call_recomputes_its_shard_before_the_gather():
    """ utils.distributed.ShardedModel: the rank's shard is checked (and, after an event, recomputed at float32) before it goes on the wire """
    from keras_retinanet_3D.utils import distributed as D
    w = scaled_weights()
    model = models.load_model(w, backbone_name='resnet50', dtype='f16x3')
    got = D.ShardedModel(model).predict_on_batch(inputs())                # (no process group: one rank holds the whole batch)
    want = models.load_model(w, backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())
    assert model.range_fallbacks == 1 and same(got, want)
    sane = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
    a = D.ShardedModel(sane).predict_on_batch(inputs())
    b = sane.predict_on_batch(inputs())
    assert sane.range_fallbacks == 0 and same(a, b)


def test_two_models_on_two_streams_only_the_affected_one_falls_back(f32_of_the_base_weights):
    """ every plan counts its range events into a slot of its own (gpp_conv_desc.range_counter, Plan.range_slot): a model whose activations
    leave the half range beside a sane one -- interleaved calls on two streams of one device, resets of either -- makes exactly its own
    calls fall back; the sane model never does, and its counters never move """
    import torch
    bad = models.load_model(scaled_weights(), backbone_name='resnet50', dtype='f16x3')
    sane = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
    want_bad = models.load_model(scaled_weights(), backbone_name='resnet50', dtype='f32').predict_on_batch(inputs())
    want_sane = sane.predict_on_batch(inputs())
    assert sane.range_fallbacks == 0
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for k in range(3):
        with torch.cuda.stream(s1):
            plan_bad = bad.stage_inputs(inputs())
            bad.run_plan(plan_bad)
        with torch.cuda.stream(s2):
            plan_sane = sane.stage_inputs(inputs())
            sane.run_plan(plan_sane)
        with torch.cuda.stream(s2):
            got_sane = sane.fetch(plan_sane)
        with torch.cuda.stream(s1):
            got_bad = bad.fetch(plan_bad)
        assert same(got_sane, want_sane) and same(got_bad, want_bad)
        assert bad.range_fallbacks == k + 1 and sane.range_fallbacks == 0
        if k == 1:
            assert bad.x3_range_events(reset=True) > 0         # a reset of one model's counters is invisible to the other
    assert sane.x3_range_events() == 0 and sane._twin is None
    assert same(f32_of_the_base_weights, want_bad)


def test_the_float32_twin_can_be_built_ahead_of_the_first_event():
    """ load_model(..., on_range_event='f32') builds its float32 twin inside the first affected call (weights upload, plan, tuning: seconds);
    prepare_fallback() does that ahead of time, and the host copy of the weights is released once the twin exists """
    model = models.load_model(scaled_weights(), backbone_name='resnet50', dtype='f16x3')
    assert model._twin is None and model._weights is not None
    model.prepare_fallback(B, H, Wd, 100, True)
    assert model._twin is not None and model._weights is None and (B, H, Wd, 100, True) in model._twin._plans
    out = model.predict_on_batch(inputs())
    assert model.range_fallbacks == 1 and int((out[2] > 0.05).sum()) > 0


# ---------------------------------------------------------------------------------------------------- every other synchronous call
# match_on_frames, the pose calls, the composites and the ragged forms of them answer a range event through the same path as
# predict_on_batch (RetinaNet3D._answer): each returns, byte for byte, what a dtype='f32' model of the same weights returns for the call.
def bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def noise_frames(shapes, seeds):
    # (black / white noise, as tests/test_draw_gpu.py feeds the synthetic weights.  Their scores lie around the 0.05 thresholds: the
    # seeds below are those whose frame keeps a detection above them at float32, so that no comparison is between empty results)
    return [(np.random.default_rng(seed).integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8) for seed, (h, w) in zip(seeds, shapes)]


def calibration(shapes, min_side=800, max_side=1333):
    from keras_retinanet_3D.utils import image
    scales = [image.compute_resize_scale((h, w, 3), min_side, max_side) for h, w in shapes]
    P_inv = np.stack([np.linalg.pinv(np.diag([s, s, 1.0]).dot(synthetic.KITTI_LIKE_P2)) for s in scales]).astype(np.float32)
    return P_inv, np.tile(synthetic.load_plane_database('100').astype(np.float32)[None], (len(shapes), 1, 1))


@pytest.fixture(scope='module')
def f32_model():
    """ the dtype='f32' model of the scaled weights; its pose stage changes none of the 8 outputs, so it answers every call below """
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('GPP_AUTOTUNE', '0')                          # (a tile never changes a byte: tests/test_network_gpu.py)
        yield models.load_model(scaled_weights(), backbone_name='resnet50', dtype='f32', pose=True)


def watched_model(**kwargs):
    return models.load_model(scaled_weights(), backbone_name='resnet50', dtype='f16x3', **kwargs)


def small_frames_and_annotations(f32_model):
    """ two 48x80 frames for the 96x160 plan, and two or three annotation rows per image made from the f32 model's own detections as
    tests/test_eval_gpu.py makes them """
    from test_eval_gpu import labels_from_rows
    from keras_retinanet_3D.utils import eval as gpp_eval
    frames = np.stack(noise_frames([(48, 80)] * B, (50, 51)))
    P_inv, planes = calibration([(48, 80)] * B, 96, 160)
    plan, scale = f32_model.stage_frames(frames, P_inv, planes, 96, 160)
    assert tuple(plan.images.shape) == (B, 96, 160, 3)
    f32_model.run_plan(plan)
    outputs = f32_model.fetch(plan)
    annotations = [labels_from_rows(gpp_eval._image_rows(outputs, k, scale, 0.05, 100))[:3] for k in range(B)]
    assert all(2 <= len(a) <= 3 for a in annotations)
    return (frames, P_inv, planes, annotations), {'min_side': 96, 'max_side': 160}


def test_match_on_frames_is_answered_by_the_twin(f32_model):
    args, sides = small_frames_and_annotations(f32_model)
    model = watched_model()
    got, scale = model.match_on_frames(*args, **sides)
    assert model.range_fallbacks == 1
    want, want_scale = f32_model.match_on_frames(*args, **sides)
    assert scale == want_scale and len(got) == len(want) == 4
    for g, w in zip(got, want):                                  # table, scores, errors, counts
        assert bytes_equal(g, w)
    assert (got[0][:, :, 1] == 1).any()                          # (some detection hits an annotation: the tables are not empty)


POSE_FRAMES = [(24, 80)] * B                                     # resize to 400x1333: the smallest plan of the calls without size arguments
POSE_SEEDS = (3, 40)


def labels_from_pose_rows(rows, counts):
    """ per image: KITTI label rows (n, 16) made from every fourth of its pose rows, slightly moved """
    from kitti_oracle import make_label
    labels = []
    for b in range(len(rows)):
        mine = [r.astype(np.float64) for r in rows[b, :counts[b]:4] if np.isfinite(r).all()]
        labels.append(np.array([make_label(kind=0, box=r[26:30] + 1.0, hwl=(r[30] * 1.02, r[17] * 0.99, r[18] * 1.01), xyz=(r[19] + 0.1, r[31], r[21] - 0.1),
                                           ry=r[32] + 0.02, alpha=r[25] + 0.1) for r in mine], np.float64).reshape(-1, 16))
    return labels


def test_pose_rows_and_their_kitti_overlaps_are_answered_by_the_twin(f32_model):
    frames = np.stack(noise_frames(POSE_FRAMES, POSE_SEEDS))
    P_inv, planes = calibration(POSE_FRAMES)
    model = watched_model(pose=True)
    (rows, counts), scale = model.predict_poses_on_frames(frames, P_inv, planes)
    assert model.range_fallbacks == 1
    (want_rows, want_counts), want_scale = f32_model.predict_poses_on_frames(frames, P_inv, planes)
    assert scale == want_scale and bytes_equal(rows, want_rows) and bytes_equal(counts, want_counts)
    assert counts.min() > 0
    labels = labels_from_pose_rows(want_rows, want_counts)
    assert sum(len(g) for g in labels) > 0
    chunk, _ = model.score_poses_on_frames(frames, P_inv, planes, labels)
    assert model.range_fallbacks == 2
    want_chunk, _ = f32_model.score_poses_on_frames(frames, P_inv, planes, labels)
    assert bytes_equal(chunk.rows.cpu().numpy(), want_chunk.rows.cpu().numpy()) and bytes_equal(chunk.rows.cpu().numpy(), want_rows)
    assert bytes_equal(chunk.overlaps.cpu().numpy(), want_chunk.overlaps.cpu().numpy())


def test_composites_are_answered_by_the_twin(f32_model):
    frames = np.stack(noise_frames(POSE_FRAMES, POSE_SEEDS))
    P_inv, planes = calibration(POSE_FRAMES)
    P_raw = np.stack([synthetic.KITTI_LIKE_P2] * B)
    model = watched_model(pose=True)
    (rows, counts), scale, pictures = model.predict_composites_on_frames(frames, P_inv, planes, P_raw, 0.05)
    assert model.range_fallbacks == 1
    (want_rows, want_counts), want_scale, want_pictures = f32_model.predict_composites_on_frames(frames, P_inv, planes, P_raw, 0.05)
    assert scale == want_scale and bytes_equal(rows, want_rows) and bytes_equal(counts, want_counts)
    assert len(pictures) == len(want_pictures) == B
    for got, want in zip(pictures, want_pictures):
        assert bytes_equal(got, want)
    assert any(not np.array_equal(p, np.vstack((f, f))) for p, f in zip(pictures, frames))       # (something was drawn)


def test_a_ragged_batch_of_images_is_answered_by_the_twin(f32_model):
    """ a list of float images of one height class: the twin is staged from the plan's canvas and heights (stage_canvas) """
    from keras_retinanet_3D.utils import image
    heights = [93, 96]
    assert image.class_height_range(24) == (93, 96) and len(set(image.class_of_resized(h, Wd) for h in heights)) == 1
    rng = np.random.default_rng(70)
    images = [rng.integers(0, 256, size=(h, Wd, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32) for h in heights]
    _, P_inv, planes = inputs()
    model = watched_model()
    out = model.predict_on_batch([images, P_inv, planes])
    assert model.range_fallbacks == 1 and model._last_plan.ragged and model._twin._last_plan.ragged
    assert same(out, f32_model.predict_on_batch([images, P_inv, planes]))
    assert int((out[2] > 0.05).sum()) > 0


def test_a_ragged_batch_of_frames_is_answered_by_the_twins_pose_rows(f32_model):
    from keras_retinanet_3D.utils import image
    shapes = [(24, 80), (43, 144)]
    cls, heights, _, _ = image.ragged_taps(shapes)               # (one class, or ValueError)
    assert cls == (100, 1333) and len(set(heights.tolist())) == 2
    frames = noise_frames(shapes, (3, 38))
    P_inv, planes = calibration(shapes)
    model = watched_model(pose=True)
    (rows, counts), scales = model.predict_poses_on_frames(frames, P_inv, planes)
    assert model.range_fallbacks == 1 and model._last_plan.ragged and model._twin._last_plan.ragged
    (want_rows, want_counts), want_scales = f32_model.predict_poses_on_frames(frames, P_inv, planes)
    assert np.array_equal(scales, want_scales) and bytes_equal(rows, want_rows) and bytes_equal(counts, want_counts)
    assert counts.min() > 0


def test_raise_refuses_the_pose_call_and_the_matching(f32_model):
    posed = watched_model(pose=True, on_range_event='raise')
    P_inv, planes = calibration(POSE_FRAMES)
    with pytest.raises(hip.GppError, match='half range'):
        posed.predict_poses_on_frames(np.stack(noise_frames(POSE_FRAMES, POSE_SEEDS)), P_inv, planes)
    assert posed.range_fallbacks == 1 and posed._twin is None
    args, sides = small_frames_and_annotations(f32_model)
    strict = watched_model(on_range_event='raise')
    with pytest.raises(hip.GppError, match='half range'):
        strict.match_on_frames(*args, **sides)
    assert strict.range_fallbacks == 1 and strict._twin is None
