"""
GPU parity of the whole predict_on_batch path against the CPU oracle.

Conv stack (floating point, "parity unpinned" w.r.t. the reference: no keras_resnet / TF here):
  * against the oracle in 16-bit storage mode (same folded + rounded weights, same rounding of every
    stored activation, float32 accumulation).  Only summation order separates the two, but a 1-ulp
    (2^-8 relative) flip of one stored activation re-rounds everything downstream, so after ~60
    layers the two bf16 computations differ by about one bf16 ulp per element -- the same distance
    the bf16 oracle has from the float32 oracle.  Tolerance (stated, O(1) head outputs):
    relative RMS error < 1 %, max abs < 0.1, median abs < 0.01;
  * against the float32 literal-BatchNormalization oracle: relative RMS < 1.5 %, max abs < 0.25.
  The tight per-layer bound on identical inputs: test_every_layer_on_oracle_inputs below (every op of
  the real graph fed with the oracle's own tensors: one rounding step) and tests/test_conv_gpu.py.
Decode + polling (integer / op-by-op float32 work): bit-exact against the oracle on the GPU's own
head tensors, which pins the plumbing between the stages.
"""
import numpy as np
import pytest
import torch

import helpers
from oracle import decode_np, net_torch, polling_np
from keras_retinanet_3D import models
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import anchors as A
from keras_retinanet_3D.utils import ledger, synthetic

pytestmark = pytest.mark.gpu

MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def images(batch, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(batch, h, w, 3)).astype(np.float32) - MEAN


def unfuse(reg, n_base=12):
    """ fused conv layout (B, P, 144) -> reference layout (B, A, 12) """
    B, P, _ = reg.shape
    op1 = reg[:, :, :4 * n_base].reshape(B, P, n_base, 4)
    rest = [reg[:, :, 4 * n_base + 2 * n_base * k: 4 * n_base + 2 * n_base * (k + 1)].reshape(B, P, n_base, 2) for k in range(4)]
    return np.concatenate([op1] + rest, axis=3).reshape(B, P * n_base, 12)


@pytest.fixture(scope='module')
def model50():
    return models.load_model('synthetic:1234', backbone_name='resnet50', dtype='bf16')


@pytest.mark.parametrize('batch,h,w', [(2, 96, 160), (1, 127, 211)])
def test_conv_stack_matches_oracle(model50, batch, h, w):
    weights = W.synthetic_weights('resnet50', 1234)
    img = images(batch, h, w, seed=h)
    planes = synthetic.load_plane_database('10').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    plan = model50.stage_inputs([img, np.tile(P_inv[None], (batch, 1, 1)), planes])
    model50.run_plan(plan)
    got = {'regression': unfuse(plan.regression.cpu().numpy()),
           'regression_dim': plan.regression_dim.cpu().numpy().reshape(batch, -1, 3),
           'classification_logits': plan.cls_logits.cpu().numpy().reshape(batch, -1, 8)}
    q = net_torch.forward(weights, img, 'resnet50', storage='bf16')
    f = net_torch.forward(weights, img, 'resnet50', storage=None)
    for key in got:
        assert got[key].shape == q[key].shape == f[key].shape
        eq = np.abs(got[key] - q[key])
        ef = np.abs(got[key] - f[key])
        centred = f[key] - f[key].mean()
        scale = np.sqrt((centred ** 2).mean())
        assert np.sqrt((eq ** 2).mean()) < 0.01 * scale and eq.max() < 0.1 and np.median(eq) < 0.01, (key, eq.max(), np.median(eq))
        assert np.sqrt((ef ** 2).mean()) < 0.015 * scale and ef.max() < 0.25, (key, ef.max())


@pytest.mark.parametrize('backbone', ['resnet50', 'resnet101', 'resnet152'])
def test_predict_on_batch_end_to_end(backbone, oracle_lib):
    batch, h, w = 2, 128, 224
    model = models.load_model('synthetic:7', backbone_name=backbone, dtype='bf16')
    img = images(batch, h, w, seed=3)
    planes = synthetic.load_plane_database('1k').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    P_inv = np.tile(P_inv[None].astype(np.float32), (batch, 1, 1))
    out = model.predict_on_batch([img, P_inv, np.tile(planes[None], (batch, 1, 1))])
    boxes, dims, scores, labels, orient, keypoints, keyplanes, residuals = out
    assert [o.shape for o in out] == [(batch, 100, 12), (batch, 100, 3), (batch, 100), (batch, 100), (batch, 100),
                                      (batch, 100, 4, 3), (batch, 100, 1, 4), (batch, 100)]
    assert labels.dtype == np.int32 and orient.dtype == np.int32 and boxes.dtype == np.float32
    assert all(o.flags.writeable for o in out)                       # run_network.py:114 does boxes /= scale
    assert (scores > 0.05).sum() > 0                                 # synthetic weights produce detections

    # decode + polling replayed by the oracle on the GPU's own head tensors: bit-exact
    plan = model.plan_for(batch, h, w, 1000, True)
    anchors = A.anchors_for_image((h, w))
    det, _ = decode_np.detect(plan.cls_logits.cpu().numpy().reshape(batch, -1, 8), unfuse(plan.regression.cpu().numpy()),
                              plan.regression_dim.cpu().numpy().reshape(batch, -1, 3), anchors)
    for got, want in zip(out[:5], det):
        assert helpers.bits_equal(got, want)
    kp, kpl, res, idx = helpers.c_oracle_poll(oracle_lib, boxes, dims, orient, P_inv, planes)
    assert helpers.bits_equal(keypoints, kp) and helpers.bits_equal(keyplanes, kpl) and helpers.bits_equal(residuals, res)
    assert np.array_equal(plan.best_index.cpu().numpy(), idx)

    # whole path on the CPU (float32 oracle) against the float32 HIP path: the same detections, orientations and plane
    # indices; then the ledger of the bf16 path against the float32 path (measured bars; tests/test_fullsize_gpu.py does the
    # same at the BASELINE size)
    m32 = models.load_model('synthetic:7', backbone_name=backbone, dtype='f32')
    out32 = m32.predict_on_batch([img, P_inv, np.tile(planes[None], (batch, 1, 1))])
    plan32 = m32.plan_for(batch, h, w, 1000, True)
    f = net_torch.forward(W.synthetic_weights(backbone, 7), img, backbone)
    det_cpu, aidx_cpu = decode_np.detect(f['classification_logits'], f['regression'], f['regression_dim'], anchors)
    kp_c, kpl_c, res_c, idx_c = helpers.c_oracle_poll(oracle_lib, det_cpu[0], det_cpu[1], det_cpu[4], P_inv, planes)
    led = ledger.parity_ledger(list(det_cpu) + [kp_c, kpl_c, res_c], aidx_cpu, idx_c,
                               out32, plan32.anchor_index.cpu().numpy(), plan32.best_index.cpu().numpy())
    assert led['detection_set_agreement'] == 1.0 and led['orientation_agreement'] == 1.0 and led['plane_index_agreement'] == 1.0, led
    assert led['max_keypoint_dev_m_within_100m'] <= 1e-3 and led['max_keypoint_rel_dev'] <= 1e-4, led
    led16 = ledger.parity_ledger(out32, plan32.anchor_index.cpu().numpy(), plan32.best_index.cpu().numpy(),
                                 out, plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy())
    print(backbone, 'bf16 vs f32:', led16)
    # measured at this size (resnet50 / 101 / 152): sets 0.85 / 0.83 / 0.84, plane index 0.92 / 0.72 (39 detections) / 0.81
    assert led16['detection_set_agreement'] >= 0.75 and led16['plane_index_agreement'] >= 0.6 and led16['orientation_agreement'] >= 0.99, led16


def test_deterministic_and_shared_planes(model50):
    batch, h, w = 2, 96, 160
    img = images(batch, h, w, seed=11)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    P_inv = np.tile(P_inv[None].astype(np.float32), (batch, 1, 1))
    a = model50.predict_on_batch([img, P_inv, np.tile(planes[None], (batch, 1, 1))])
    b = model50.predict_on_batch([img, P_inv, planes])                # (N, 4) database shared by the batch
    c = model50.predict_on_batch([img, P_inv, np.tile(planes[None], (batch, 1, 1))])
    for x, y, z in zip(a, b, c):
        assert helpers.bits_equal(x, y) and helpers.bits_equal(x, z)


def test_model_loaded_from_a_keras_h5_checkpoint(model50, tmp_path):
    """ the reference's checkpoint format (bin/convert_model.py:50-53 -> models/__init__.py:81): a model loaded from an .h5 in
    the Keras layout returns the bytes of the model built from the same arrays in memory """
    from keras_retinanet_3D.models import hdf5
    try:
        hdf5.library()
    except hdf5.Hdf5Error as e:
        pytest.skip(str(e))
    path = str(tmp_path / 'resnet50_inference.h5')
    W.save_weights(path, W.synthetic_weights('resnet50', 1234))
    model = models.load_model(path, backbone_name='resnet50', convert=False, dtype='bf16')
    batch, h, w = 2, 96, 160
    img = images(batch, h, w, seed=21)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    P_inv = np.tile(P_inv[None].astype(np.float32), (batch, 1, 1))
    a = model.predict_on_batch([img, P_inv, planes])
    b = model50.predict_on_batch([img, P_inv, planes])
    assert (a[2] > 0.05).sum() > 0
    for x, y in zip(a, b):
        assert helpers.bits_equal(x, y)


def test_decode_overlap_does_not_change_results(monkeypatch):
    """ default plan: classification + regression towers first, detection selection on a side stream underneath the
    dimension tower; GPP_DECODE_OVERLAP=0: the serial order.  Same kernels, same inputs: identical outputs.
    (Both models tune their block tiles by timing, independently: tiles never change a result, split-K is a rule.) """
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    x = images(2, 160, 256, seed=9)
    P = np.tile(P_inv[None].astype(np.float32), (2, 1, 1))
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='bf16')
    got = model.predict_on_batch([x, P, np.tile(planes[None], (2, 1, 1))])
    plan = model.plan_for(2, 160, 256, planes.shape[0], True)
    assert plan.decode_overlap and [op[3] for op in plan.ops if op[3].startswith('filtered')] == \
        ['filtered_detections/candidates', 'filtered_detections/select', 'filtered_detections']
    monkeypatch.setenv('GPP_DECODE_OVERLAP', '0')
    serial = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='bf16')
    want = serial.predict_on_batch([x, P, np.tile(planes[None], (2, 1, 1))])
    assert not serial.plan_for(2, 160, 256, planes.shape[0], True).decode_overlap
    assert (got[2] > 0.05).sum() > 0
    for a, b in zip(got, want):
        assert helpers.bits_equal(a, b)
    for _ in range(3):                       # back-to-back runs reuse the side stream and the workspace
        again = model.predict_on_batch([x, P, np.tile(planes[None], (2, 1, 1))])
        for a, b in zip(again, want):
            assert helpers.bits_equal(a, b)


@pytest.mark.parametrize('dtype', ['f16x3', 'bf16'])
def test_side_stream_lanes_do_not_change_results(dtype, monkeypatch):
    """ default plan: res2 .. res5 as two half batches (1 + 2 images here) on two streams (a stage that is NOT split puts the projection shortcut of its
    first block on a side stream beside branch2a / 2b: GPP_HALF_LANES=1,2,3 in the plan-variant test below), P5 and the
    P6 -> ReLU -> P7 chain beside C4_reduced, P4 (behind P5) beside C3_reduced / P3.  GPP_BR1_LANE=0 GPP_FPN_LANES=0: everything on one stream.  Disjoint outputs,
    explicit joins: identical bytes, head tensors and pyramid included, also on repeated runs. """
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    x = images(3, 200, 333, seed=12)
    P = np.tile(P_inv[None].astype(np.float32), (3, 1, 1))
    inputs = [x, P, np.tile(planes[None], (3, 1, 1))]

    def run(n=1):
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype=dtype)
        outs = []
        for _ in range(n):
            out = model.predict_on_batch(inputs)
            plan = model.plan_for(3, 200, 333, planes.shape[0], True)
            outs.append(out + [plan.cls_logits.cpu().numpy(), plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy()] +
                        [plan.features[k].buf.contiguous().view(torch.uint8).cpu().numpy() for k in ('C3', 'C4', 'C5', 'P3')])
        return outs, plan

    lanes, plan = run(4)
    assert plan.side_lanes == {'fpn': True, 'branch1': True, 'p4': True, 'half_batch_stages': [0, 1, 2, 3], 'cls_tower': False}
    names = [op[3] for op in plan.ops]
    assert names.count('res4b_branch2b') == 2 and names.count('res2a_branch2a') == 2      # one launch per half batch (res2 too since round 6)
    monkeypatch.setenv('GPP_BR1_LANE', '0')
    monkeypatch.setenv('GPP_FPN_LANES', '0')
    monkeypatch.setenv('GPP_HALF_LANES', '')
    serial, splan = run()
    assert splan.side_lanes == {'fpn': False, 'branch1': False, 'p4': False, 'half_batch_stages': [], 'cls_tower': False}
    assert (serial[0][2] > 0.05).sum() > 0
    for got in lanes:
        for a, b in zip(got, serial[0]):
            assert helpers.bits_equal(a, b)


PLAN_OPTIONS = helpers.PLAN_OPTIONS


# the default GPU run keeps the settings that changed a plan's shape in a way of its own (the default, the split / unsplit pattern of the round-4 race,
# towers on side streams, chunked stages, no half batches); the rest of the matrix runs under --run-slow (tools/collect_r5.sh)
PLAN_OPTIONS_DEFAULT_RUN = (0, 1, 10, 15, 17, 18)


@pytest.mark.parametrize('options', [o if i in PLAN_OPTIONS_DEFAULT_RUN else pytest.param(o, marks=pytest.mark.slow) for i, o in enumerate(PLAN_OPTIONS)],
                         ids=[' '.join('{}={}'.format(*kv) for kv in o.items()) or 'default' for o in PLAN_OPTIONS])
def test_every_plan_variant_orders_its_streams_and_gives_the_same_bytes(options, monkeypatch):
    """ The plan builder puts launches on side streams by hand (half batches of res3-res5, projection shortcuts, small FPN launches,
    the detection selection).  Plan.check_stream_ordering replays gpp_plan_run's fork / join rules over the bytes every launch reads and
    writes: two launches on different streams that touch the same bytes (one of them writing) must have a fork or a join between
    them.  Round 4 found a missing join this way of thinking would have caught: a stage that ran as two half batches followed by one
    that did not (GPP_HALF_LANES=1,2) read the second half's maps unjoined -- a race that only showed at full size, and only in a
    non-default configuration the earlier rounds had used for timing.  Every switch the builder has is checked here, and each variant
    must return the bytes of the one-stream plan. """
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    x = images(4, 200, 333, seed=12)
    P = np.tile(P_inv[None].astype(np.float32), (4, 1, 1))
    inputs = [x, P, np.tile(planes[None], (4, 1, 1))]

    def run(env):
        for k in ('GPP_HALF_LANES', 'GPP_BR1_LANE', 'GPP_FPN_LANES', 'GPP_P4_LANE', 'GPP_HEAD_LANES', 'GPP_DECODE_OVERLAP', 'GPP_STAGE_CHUNKS', 'GPP_CLS_LANE', 'GPP_FUSE_BLOCK', 'GPP_FUSE_BLOCK_PROJ'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
        out = model.predict_on_batch(inputs)
        plan = model.plan_for(4, 200, 333, planes.shape[0], True)
        extra = [plan.cls_logits.cpu().numpy(), plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy()]
        return out + extra, plan

    got, plan = run(options)
    assert plan.check_stream_ordering() == []
    serial, splan = run({'GPP_HALF_LANES': '', 'GPP_BR1_LANE': '0', 'GPP_FPN_LANES': '0', 'GPP_DECODE_OVERLAP': '0', 'GPP_CLS_LANE': '0'})
    assert splan.check_stream_ordering() == [] and all((f >> 8) & 0xff == 0 for f in splan.lanes)        # everything on the caller's stream
    for a, b in zip(got, serial):
        assert helpers.bits_equal(a, b)


def test_the_stream_ordering_check_sees_a_missing_join(monkeypatch):
    """ the checker itself: take the join away from the launch that consumes the half-batch lanes, or the fork (SYNC) from a side launch
    that reads what the main stream has just written, and it says so """
    from keras_retinanet_3D.models import retinanet as R
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
    plan = model.plan_for(4, 200, 333, 100, True)
    assert plan.check_stream_ordering() == []
    names = [op[3] for op in plan.ops]
    i = names.index('C5_reduced')
    assert plan.lanes[i] & R.OP_JOIN
    saved = plan.lanes[i]
    plan.lanes[i] &= ~R.OP_JOIN
    bad = plan.check_stream_ordering()
    assert bad and any(later == 'C5_reduced' for _, later in bad)
    plan.lanes[i] = saved
    i = names.index('P4')
    assert plan.lanes[i] & R.OP_SYNC
    plan.lanes[i] &= ~R.OP_SYNC
    assert any(later == 'P4' for _, later in plan.check_stream_ordering())


@pytest.mark.parametrize('dtype', [pytest.param('bf16', marks=pytest.mark.slow), 'f16x3'])
def test_random_tiles_never_change_a_byte(dtype, monkeypatch):
    """ GPP_TUNE_RANDOM: every conv layer (and fused tail) of the plan takes a RANDOM tile among the autotuner's candidates
    (gpp_conv2d_tile_candidates) instead of the fastest one -- three different draws and the measured choice give identical output
    bytes, head tensors included: the block tile never changes the K order of an output element (split-K is a rule of the layer) """
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    x = images(2, 200, 333, seed=4)
    P = np.tile(P_inv[None].astype(np.float32), (2, 1, 1))
    inputs = [x, P, np.tile(planes[None], (2, 1, 1))]

    def run():
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype=dtype)
        out = model.predict_on_batch(inputs)
        plan = model.plan_for(2, 200, 333, planes.shape[0], True)
        return out + [plan.cls_logits.cpu().numpy(), plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy()], dict(plan.tuning)

    want, tuned = run()
    assert (want[2] > 0.05).sum() > 0
    draws = []
    for seed in (1, 2, 3):
        monkeypatch.setenv('GPP_TUNE_RANDOM', str(seed))
        got, tiles = run()
        draws.append(tiles)
        for a, b in zip(got, want):
            assert helpers.bits_equal(a, b), seed
    assert draws[0] != draws[1] or draws[1] != draws[2]            # the draws really differ
    assert any(draws[0][k][0] != tuned[k][0] for k in tuned)


def test_the_tune_cache_carries_every_choice_from_one_model_to_the_next(tmp_path, monkeypatch):
    """ GPP_TUNE_CACHE across two models of one process, on the smallest plan whose cache holds every kind of key (resnet50 f16x3, B = 4,
    224 x 352, both round thresholds at 0): half-batch layers, a fused tail's row count, a guarded pair's and a tower layer's '@rows' key.
    The first model times its layers and writes the file; the second finds every choice there -- the same plan.tuning, the file's bytes
    untouched, the same output bytes; an entry edited to a tile its layer does not list is timed again, never launched """
    import json
    path = tmp_path / 'tile_choices.json'
    monkeypatch.setenv('GPP_TUNE_CACHE', str(path))
    monkeypatch.setenv('GPP_SPARSE_TOWER_MIN_ROUNDS', '0')
    monkeypatch.setenv('GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS', '0')
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    inputs = [images(4, 224, 352, seed=5), np.tile(P_inv[None].astype(np.float32), (4, 1, 1)), np.tile(planes[None], (4, 1, 1))]

    def run():
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
        out = model.predict_on_batch(inputs)
        plan = model.plan_for(4, 224, 352, planes.shape[0], True)
        return out + [plan.cls_logits.cpu().numpy(), plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy()], plan

    want, first = run()
    assert (want[2] > 0.05).sum() > 0 and len(first.sparse.gathered) == 2 and len(first.sparse.tower) == 1 and first.sparse.deep_layers == 2
    written = path.read_bytes()
    keys = [k.split('|') for k in json.loads(written)]
    assert all(len(k) == 7 and k[1:3] == ['resnet50', 'f16x3'] and k[5:] == ['224', '352'] for k in keys)
    layers = {(k[3], int(k[4])) for k in keys}
    assert {('res4a_branch2a', 2), ('res2a_branch2b+2c', 2), ('P3', 4), ('pyramid_regression_ops', 4), ('pyramid_regression_ops@rows', 4),
            ('pyramid_regression_dim@rows', 4), ('pyramid_regression_3', 4), ('pyramid_regression_3@rows', 4)} <= layers
    assert {name for name, _ in layers} == set(first.tuning)
    got, second = run()
    assert second is not first and second.tuning == first.tuning and second.tuning_parts == first.tuning_parts
    assert path.read_bytes() == written                          # nothing was timed again
    for a, b in zip(got, want):
        assert helpers.bits_equal(a, b)
    data = json.loads(written)
    edited = next(k for k in data if k.split('|')[3:5] == ['P3', '4'])
    data[edited] = [0x7fffffff, 1.0]
    path.write_text(json.dumps(data))
    got, third = run()
    assert third.tuning['P3'][0] != 0x7fffffff and third.tuning['P3'][0] == json.loads(path.read_text())[edited][0]
    assert {k: v for k, v in third.tuning.items() if k != 'P3'} == {k: v for k, v in first.tuning.items() if k != 'P3'}
    for a, b in zip(got, want):
        assert helpers.bits_equal(a, b)


def test_hip_graph_capture_replays_the_plan(monkeypatch):
    """ model.capture(plan): the whole plan, side-stream fork / join of the detection selection included, recorded into a
    HIP graph; replays give the eager results bit for bit on new inputs """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='bf16')
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    P = np.tile(P_inv[None].astype(np.float32), (2, 1, 1))
    pl = np.tile(planes[None], (2, 1, 1))
    x0, x1 = images(2, 160, 256, seed=3), images(2, 160, 256, seed=4)
    want0 = model.predict_on_batch([x0, P, pl])
    want1 = model.predict_on_batch([x1, P, pl])
    assert not all(helpers.bits_equal(a, b) for a, b in zip(want0, want1))
    plan = model.plan_for(2, 160, 256, planes.shape[0], True)
    assert plan.decode_overlap
    model.capture(plan)
    for x, want in ((x0, want0), (x1, want1), (x0, want0)):
        got = model.predict_on_batch([x, P, pl])
        for a, b in zip(got, want):
            assert helpers.bits_equal(a, b)


def test_orientation_specific_filter_through_the_model(monkeypatch):
    """ models.load_model(..., orientation_specific_filter=True): same conv stack, per-orientation decode; checked against the
    oracle's decode of the GPU's own head tensors, then polling against the C oracle """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    model = models.load_model('synthetic:1234', backbone_name='resnet50', orientation_specific_filter=True, dtype='bf16')
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    x = images(2, 160, 256, seed=5)
    P = np.tile(P_inv[None].astype(np.float32), (2, 1, 1))
    out = model.predict_on_batch([x, P, np.tile(planes[None], (2, 1, 1))])
    plan = model.plan_for(2, 160, 256, planes.shape[0], True)
    assert not plan.decode_overlap
    cls = plan.cls_logits.cpu().numpy().reshape(2, -1, 8)
    reg12 = unfuse(plan.regression.cpu().numpy())
    det, _ = decode_np.detect(cls, reg12, plan.regression_dim.cpu().numpy().reshape(2, -1, 3), A.anchors_for_image((160, 256)),
                              orientation_specific_filter=True)
    assert (det[2] > 0.05).sum() > 0
    for got, want in zip(out[:5], det):
        assert helpers.bits_equal(got, want)
    kp, kpl, res = polling_np.fit_road_planes(out[0], out[1], out[4], P, np.tile(planes[None], (2, 1, 1)))
    assert np.array_equal(out[6], kpl) and np.allclose(out[5], kp, atol=1e-4) and np.allclose(out[7], res, atol=1e-5)


def test_pack_kernel_equals_the_torch_concatenation(model50):
    """ gpp_pack_detections (one launch) == torch.cat of the eight arrays; unpack restores them exactly """
    import torch
    from keras_retinanet_3D.utils import distributed as D
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    x = images(2, 160, 256, seed=2)
    out = model50.predict_on_batch([x, np.tile(P_inv[None].astype(np.float32), (2, 1, 1)), np.tile(planes[None], (2, 1, 1))])
    plan = model50.plan_for(2, 160, 256, planes.shape[0], True)
    dev_outs = model50.outputs(plan)
    packed = D.pack_outputs(dev_outs)
    ref = torch.cat([o.reshape(2, 100, -1).to(torch.float32) for o in dev_outs], dim=2)
    assert packed.shape == (2, 100, 35) and torch.equal(packed.cpu().view(torch.int32), ref.cpu().view(torch.int32))
    for a, b in zip(D.unpack_outputs(packed), out):
        assert a.dtype == b.dtype and helpers.bits_equal(a, b) if a.dtype.kind == 'f' else np.array_equal(a, b)


def test_f16_storage_runs_and_agrees_with_bf16(model50):
    batch, h, w = 1, 96, 160
    img = images(batch, h, w, seed=5)
    planes = synthetic.load_plane_database('10').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    m16 = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16')
    p1 = model50.stage_inputs([img, P_inv[None], planes]); model50.run_plan(p1)
    p2 = m16.stage_inputs([img, P_inv[None], planes]); m16.run_plan(p2)
    q = net_torch.forward(W.synthetic_weights('resnet50', 1234), img, 'resnet50', storage='f16')
    got = p2.cls_logits.cpu().numpy().reshape(batch, -1, 8)
    assert np.abs(got - q['classification_logits']).max() < 5e-3
    assert np.abs(got - p1.cls_logits.cpu().numpy().reshape(batch, -1, 8)).max() < 0.1


def test_bad_inputs_raise(model50):
    with pytest.raises(ValueError):
        model50.predict_on_batch([np.zeros((1, 64, 64, 4), np.float32), np.zeros((1, 4, 3), np.float32), np.ones((4, 4), np.float32)])
    with pytest.raises(ValueError):
        model50.predict_on_batch([np.zeros((1, 64, 64, 3), np.float32), np.zeros((2, 4, 3), np.float32), np.ones((4, 4), np.float32)])
    with pytest.raises(ValueError):
        models.load_model('synthetic:1', backbone_name='resnet34')        # models/resnet.py:61-68
    with pytest.raises(NotImplementedError):
        models.load_model('synthetic:1', backbone_name='vgg16')           # out of scope


def test_run_network_cli_on_the_gpu(tmp_path):
    """ the real CLI end to end: PNG + calibration files in, .mat + KITTI files out (synthetic weights) """
    import scipy.io
    from PIL import Image
    from keras_retinanet_3D.bin import run_network
    (tmp_path / 'img').mkdir(); (tmp_path / 'calib').mkdir(); (tmp_path / 'out').mkdir()
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    for k in range(3):
        # binary noise: keeps enough contrast through the bilinear resize for the synthetic weights (calibrated on
        # full-contrast noise) to put anchors above the 0.05 score threshold
        frame = (np.random.default_rng(k).integers(0, 2, size=(375, 1242, 3)) * 255).astype(np.uint8)
        Image.fromarray(frame[:, :, ::-1]).save(str(tmp_path / 'img' / ('%06d.png' % k)))
        (tmp_path / 'calib' / ('%06d.txt' % k)).write_text(calib)
    run_network.main(['synthetic:1234.h5', str(tmp_path / 'img'), str(tmp_path / 'calib'), synthetic.plane_database_path('1k'),
                      str(tmp_path / 'out'), '--kitti', '--batch-size', '2'])
    for k in range(3):
        mat = scipy.io.loadmat(str(tmp_path / 'out' / 'synthetic:1234' / 'outputs' / 'full' / ('%06d.mat' % k)))
        n = mat['scores'].shape[1]
        assert n > 0 and mat['boxes'].shape == (n, 4) and mat['keypoints'].shape == (n, 8) and mat['locations'].shape == (n, 3)
        assert np.all(np.diff(mat['scores'][0]) <= 0) and np.isfinite(mat['angles']).all()
        txt = (tmp_path / 'out' / 'synthetic:1234' / 'outputs' / 'kitti' / ('%06d.txt' % k)).read_text()
        assert txt.count('\n') == n and txt.startswith('Car -1 -1 ')


def test_evaluate_cli_on_the_gpu(tmp_path, model50):
    """ utils.eval.evaluate through the real model on a KITTI-style directory: ground truth is taken from the model's own
    detections of two frames (every second one, original pixel units), so the matching, AP and error code see real
    GPU outputs; evaluation is deterministic and batched evaluation agrees with one-at-a-time evaluation """
    import scipy.io
    from PIL import Image
    from keras_retinanet_3D.bin import evaluate as evaluate_cli
    from keras_retinanet_3D.preprocessing.kitti import KittiGenerator
    from keras_retinanet_3D.utils import eval as gpp_eval, image
    base = tmp_path / 'kitti'
    for d in ('images', 'labels', 'calibs'):
        (base / 'val' / d).mkdir(parents=True)
    planes = synthetic.load_plane_database('100')
    scipy.io.savemat(str(base / 'road_planes_database.mat'), {'road_planes_database': planes})
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    total = 0
    for k in range(3):
        frame = (np.random.default_rng(k).integers(0, 2, size=(120, 200, 3)) * 255).astype(np.uint8)
        Image.fromarray(frame[:, :, ::-1]).save(str(base / 'val' / 'images' / ('%06d.png' % k)))
        (base / 'val' / 'calibs' / ('%06d.txt' % k)).write_text(calib)
        img, scale = image.resize_image(image.preprocess_image(image.read_image_bgr(str(base / 'val' / 'images' / ('%06d.png' % k)))))
        P_inv = np.linalg.pinv(np.diag([scale, scale, 1.0]).dot(P2))
        out = model50.predict_on_batch([img[None], P_inv[None], planes[None]])
        lines = []
        for d in range(0, int((out[2][0] > 0.05).sum()), 2):
            b = out[0][0, d] / scale
            lines.append('Car 0.00 0 0.00 ' + ' '.join('%.4f' % v for v in b) + ' ' + ' '.join('%.4f' % v for v in out[1][0, d]) +
                         ' %d' % out[4][0, d])
        total += len(lines)
        (base / 'val' / 'labels' / ('%06d.txt' % k)).write_text('\n'.join(lines) + ('\n' if lines else ''))
    assert total > 0
    gen = KittiGenerator(str(base), subset='val')
    one = gpp_eval.evaluate(gen, model50, batch_size=1)
    many = gpp_eval.evaluate(gen, model50, batch_size=3)
    assert sorted(one[0]) == [0, 1, 2, 3] and sum(n for _, n in one[0].values()) == total
    again = gpp_eval.evaluate(gen, model50, batch_size=1)
    assert again[0] == one[0] and again[1:] == one[1:]                # deterministic
    for label in one[0]:
        # another batch size is another plan with its own tile choices -- which never change a result (split-K follows a
        # rule of the layer alone): batched evaluation equals one-at-a-time evaluation exactly
        assert one[0][label] == many[0][label]
    assert max(ap for ap, n in one[0].values() if n > 0) > 0.3        # its own detections are found again
    assert one[1] < 1e-3 and one[2] < 1e-3                            # matched keypoints / heights equal the labels (%.4f)
    logs = evaluate_cli.main(['synthetic:1234.h5', str(base), '--batch-size', '2'])
    assert 0.0 < logs['mAP'] <= 1.0


def test_frame_pipeline_matches_synchronous_calls(model50):
    from keras_retinanet_3D.utils.pipeline import FramePipeline
    from keras_retinanet_3D.utils import image
    planes = synthetic.load_plane_database('100').astype(np.float32)
    scale = image.compute_resize_scale((375, 1242, 3))
    _, P_inv = synthetic.synthetic_calibration(scale)
    P_inv = np.tile(P_inv[None].astype(np.float32), (2, 1, 1))
    batches = []
    for k in range(5):
        frames = (np.random.default_rng(k).integers(0, 2, size=(2, 375, 1242, 3)) * 255).astype(np.uint8)
        batches.append((frames, P_inv, planes))
    want = [model50.predict_on_frames(*b)[0] for b in batches]
    got = list(FramePipeline(model50, depth=2).run(iter(batches)))
    assert len(got) == 5
    for (outs, sc), ref in zip(got, want):
        assert sc == scale
        for a, b in zip(outs, ref):
            assert helpers.bits_equal(a, b) if a.dtype.kind == 'f' else np.array_equal(a, b)


@pytest.mark.parametrize('backbone,dtype,fuse_next', [('resnet50', 'bf16', '0'), pytest.param('resnet101', 'f16', '0', marks=pytest.mark.slow),
                                                      pytest.param('resnet152', 'bf16', '0', marks=pytest.mark.slow), ('resnet50', 'f32', '0'),
                                                      pytest.param('resnet101', 'f32', '0', marks=pytest.mark.slow),
                                                      pytest.param('resnet50', 'bf16x3', '0', marks=pytest.mark.slow),
                                                      ('resnet50', 'f16x3', '0'), ('resnet101', 'f16x3', '0')])
def test_every_layer_on_oracle_inputs(backbone, dtype, fuse_next, monkeypatch):
    check_every_layer(backbone, dtype, fuse_next, 2, 120, 200, monkeypatch)


def check_every_layer(backbone, dtype, fuse_next, batch, h, w, monkeypatch):
    """ Layer-by-layer parity over the ACTUAL graph (every conv / stem / pool / relu op of the plan, with
    its real shapes, strides, paddings, fused residuals, fused nearest-upsample, grouped pyramid
    launches): before each op its input (and residual) buffers are overwritten with the oracle's own
    tensors, so no error can propagate and the bound is tight.  Products of 16-bit operands are exact in
    float32; only the summation order differs, so a stored bf16 output may differ from the oracle's by
    one rounding step.  Tolerance: |gpu - oracle| <= ulp |oracle| + 1e-4 * rms (ulp 2^-7 bf16, 2^-10 f16) and
    >= 99 % of elements bit-equal; float32 maps (the head outputs, and EVERY map of the dtype='f32' reference-precision
    path, whose oracle is the literal-BatchNormalization float32 graph): <= 2e-5 * rms + 1e-5 |oracle|; dtype='bf16x3'
    (float32 storage, three bf16 products per float32 product) against the same float32 oracle: <= 2e-4 * rms + 1e-4 |oracle|;
    dtype='f16x3' (three IEEE-half products, 22 significant bits per operand): float32's own bar.
    (tests/test_fullsize_gpu.py runs the same check at the BASELINE size 402x1333.) """
    import torch
    from keras_retinanet_3D.models.retinanet import OP_BLOCK, OP_CONV, OP_MAXPOOL, OP_RELU, OP_STEM, OP_STEM_POOL, OP_TAIL
    monkeypatch.setenv('GPP_HALF_LANES', '')          # one launch per layer over the whole batch (the half-batch plan: same kernels on image sub-ranges,
    model50 = models.load_model('synthetic:1234', backbone_name=backbone, dtype=dtype)      # identical bytes: test_side_stream_lanes_do_not_change_results)
    weights = W.synthetic_weights(backbone, 1234)
    img = images(batch, h, w, seed=11)
    planes = synthetic.load_plane_database('10').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    plan = model50.stage_inputs([img, np.tile(P_inv[None], (batch, 1, 1)), planes])
    ref = net_torch.forward(weights, img, backbone, storage=None if dtype in ('f32', 'bf16x3', 'f16x3') else dtype, trace=True)
    tr = ref['trace']
    ulp = 1.0 / 128 if dtype == 'bf16' else 1.0 / 1024

    def oracle_of(name, level):
        if name == 'pyramid_towers_0':
            return np.concatenate([tr[('pyramid_regression_0', level)], tr[('pyramid_classification_0', level)],
                                   tr[('pyramid_regression_dim_0', level)]], axis=-1)
        if name == 'pyramid_regression_ops':
            return np.concatenate([tr[('pyramid_regression_op{}'.format(k), level)] for k in (1, 2, 3, 4, 5)], axis=-1)
        return tr[(name.replace('branch2a+2b+2c', 'branch2c').replace('branch2b+2c', 'branch2c'), level)]      # fused launches: the output of the last 1x1

    produced = {}                       # (buffer address, element offset) -> oracle array (B, H, W, C_total)

    def key(fm):
        return (fm.buf.data_ptr(), fm.off)

    def register(fm, arr):
        produced[key(fm)] = arr
        for c0 in (512, 768):            # channel slices of the wide tower-0 tensor are consumed separately
            if fm.C == 896:
                produced[(fm.buf.data_ptr(), fm.off + c0)] = arr[..., c0:]

    def feed(fm):
        arr = produced[key(fm)][..., :fm.C]
        assert arr.shape == (fm.B, fm.H, fm.W, fm.C), (arr.shape, (fm.B, fm.H, fm.W, fm.C))
        fm.write(torch.as_tensor(np.ascontiguousarray(arr)))          # (a pre-split bf16x3 map splits the values here)

    def compare(name, fm, want, slack=1e-4):
        got = fm.read().float().cpu().numpy()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        rms = float(np.sqrt((want.astype(np.float64) ** 2).mean())) + 1e-30
        err = np.abs(got - want)
        if fm.buf.dtype == torch.float32:
            k = 10.0 if dtype == 'bf16x3' else 1.0
            assert (err <= k * (2e-5 * rms + 1e-5 * np.abs(want))).all(), (name, err.max(), rms)
        else:
            assert (err <= np.abs(want) * ulp + slack * rms).all(), (name, err.max(), rms)
            assert (got == want).mean() >= 0.99, (name, (got == want).mean())

    checked = 0
    for index, (kind, _, _, name, _) in enumerate(plan.ops):
        if kind == OP_STEM:
            model50.run_op(plan, index)
            compare(name, plan.stem_out, tr[('conv1', 0)])
            register(plan.stem_out, tr[('conv1', 0)])
        elif kind == OP_STEM_POOL:                               # conv1 + pool1 in one launch: the max of the stored conv values
            model50.run_op(plan, index)
            compare(name, plan.pool_out, tr[('pool1', 0)])
            register(plan.pool_out, tr[('pool1', 0)])
        elif kind == OP_MAXPOOL:
            feed(plan.stem_out)
            model50.run_op(plan, index)
            compare(name, plan.pool_out, tr[('pool1', 0)])       # a max of stored values: exact
            assert (plan.pool_out.dense().float().cpu().numpy() == tr[('pool1', 0)]).all()
            register(plan.pool_out, tr[('pool1', 0)])
        elif kind == OP_RELU:
            src, dst = plan.relu_io
            feed(src)
            model50.run_op(plan, index)
            got_relu = dst.read().float().cpu().numpy()
            assert (got_relu == tr[('C6_relu', 0)]).all() if not dst.split else np.allclose(got_relu, tr[('C6_relu', 0)], rtol=2e-5, atol=1e-7)
            register(dst, tr[('C6_relu', 0)])
        elif kind in (OP_CONV, OP_TAIL, OP_BLOCK):
            inputs, outputs, residuals = plan.io[name]
            for fm in inputs + (residuals or []):
                feed(fm)
            model50.run_op(plan, index)
            torch.cuda.synchronize()
            for level, fm in enumerate(outputs):
                want = oracle_of(name, level if len(outputs) > 1 else 0)
                # a fused 3x3 + 1x1 launch rounds its intermediate on the GPU: a rare one-step flip there moves
                # all output channels of that pixel by ~|w| * 2^-8
                compare(name, fm, want, slack=4e-3 if kind in (OP_TAIL, OP_BLOCK) else 1e-4)
                register(fm, want)
        else:
            continue
        checked += 1
    n_decode = sum(1 for op in plan.ops if op[3].startswith('filtered_detections') or op[3] == 'fit_road_planes')
    assert n_decode in (2, 4) and checked == len(plan.ops) - n_decode     # everything but decode and polling (bit-exact tests elsewhere)
