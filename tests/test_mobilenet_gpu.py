"""
MobileNet backbones on the GPU: the fused depthwise-separable block (gpp_mobilenet_block) through the C ABI against a float64
relu6(W . relu6(dw(x) + t) + b), every tile bit-identical; the stem (gpp_mobilenet_stem) bit for bit against a NumPy float32 loop in the
documented tap order; mobilenet224_1.0 end to end against the float64 oracle of tests/mobilenet_oracle.py within the reference bars.
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import mobilenet_oracle as MO
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from keras_retinanet_3D.layers import mobilenet as M
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import ledger, synthetic

pytestmark = pytest.mark.gpu

MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def padded_taps(x, stride, Ho, Wo):
    """ the nine (B, Ho, Wo, C) views of the zero-padded input, tap dy * 3 + dx: symmetric pad 1, window origin o * stride - 1 """
    xp = np.zeros((x.shape[0], x.shape[1] + 2, x.shape[2] + 2, x.shape[3]), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return [xp[:, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride] for dy in range(3) for dx in range(3)]


def block_case(cin, cout, B, H, Wd, stride, dtype, seed=0):
    rng = np.random.default_rng(seed)
    pitch = cin + 8                                       # the input is read through a pitch
    x = np.zeros((B, H, Wd, pitch), np.float32)
    x[...] = np.clip(rng.standard_normal(x.shape) * 2.0, 0.0, 6.0)          # a post-ReLU6 map: zeros, sixes and values between
    kd = (rng.standard_normal((3, 3, cin, 1)) * 0.5).astype(np.float32)
    bd = (rng.standard_normal(cin) * 0.5).astype(np.float32)
    kp = (rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    bp = (rng.standard_normal(cout) + 2.0).astype(np.float32)
    Ho, Wo = M.out_size(H, stride), M.out_size(Wd, stride)
    dev = torch.device('cuda')
    xin = torch.as_tensor(x).to(dev)
    out = torch.zeros((B, Ho, Wo, cout), dtype=torch.float32, device=dev)
    pw, scale = M.pack_pointwise(kp, dtype, dev)
    keep = [torch.as_tensor(M.pack_depthwise(kd)).to(dev), torch.as_tensor(bd).to(dev), pw, torch.as_tensor(bp).to(dev), scale, xin, out]
    d = M.block_desc(C.FMap(xin, B, H, Wd, cin, pitch=pitch), C.FMap(out, B, Ho, Wo, cout), keep[0], keep[1], pw, keep[3], scale, stride, dtype)
    x64 = x[..., :cin].astype(np.float64)
    mid = np.clip(sum(t * kd[dy, dx, :, 0].astype(np.float64) for t, (dy, dx) in
                      zip(padded_taps(x64, stride, Ho, Wo), [(a, b) for a in range(3) for b in range(3)])) + bd, 0.0, 6.0)
    pre = mid @ kp[0, 0].astype(np.float64) + bp
    mass = mid @ np.abs(kp[0, 0]).astype(np.float64) + np.abs(bp)            # sum |x| |w| + |b| per output: the scale of rounding errors
    return d, keep, out, mid, np.clip(pre, 0.0, 6.0), mass


def run_block(d):
    hip.check(hip.lib().gpp_mobilenet_block(ctypes.byref(d), hip.stream_ptr()), 'gpp_mobilenet_block')


BLOCK_CASES = [(8, 16, (9, 13), 1), (8, 16, (10, 14), 2), (32, 64, (16, 22), 2), (32, 64, (17, 31), 1), (128, 64, (17, 31), 2),
               (128, 1024, (12, 20), 1), (1024, 1024, (6, 9), 1), (1024, 16, (7, 10), 2), (24, 48, (11, 12), 2)]


@pytest.mark.parametrize('dtype', ['f32', 'f16x3', 'bf16x3'])
@pytest.mark.parametrize('cin,cout,hw,stride', BLOCK_CASES)
def test_block_against_float64_every_tile(dtype, cin, cout, hw, stride):
    """ bars: relative 1e-5 (f32) and 2e-5 (f16x3) with denominator |ref| + 1, those of test_preact_against_float64_every_tile.
    bf16x3 (not one of the issue's cases; reasoning: x and w are each hi + lo to 2^-17 relative and the lo * lo product, < 2^-16 of
    |x| |w|, is dropped, so a product is off by less than 2^-15 |x| |w| and an output by less than 2^-15 (sum |x| |w| + |b|)). """
    d, keep, out, mid, ref, mass = block_case(cin, cout, 2, hw[0], hw[1], stride, dtype)
    assert (mid == 0).any() and (mid == 6).any() and (ref == 0).any() and (ref == 6).any()       # both clamps of both stages are reached
    tiles, count = (ctypes.c_int * 16)(), ctypes.c_int(0)
    hip.check(hip.lib().gpp_mobilenet_block_tile_candidates(ctypes.byref(d), tiles, 16, ctypes.byref(count)), 'candidates')
    assert count.value >= 4
    first = None
    for tile in tiles[:count.value]:
        d.tile_hint = tile
        out.fill_(-1.0)
        run_block(d)
        got = out.cpu().numpy()
        if first is None:
            first = got
            if dtype == 'bf16x3':
                err = np.abs(got - ref) / mass
                bar = 2.0 ** -15
            else:
                err = np.abs(got - ref) / (np.abs(ref) + 1.0)
                bar = 2e-5 if dtype == 'f16x3' else 1e-5
            print('gpp_mobilenet_block', dtype, cin, cout, hw, stride, 'max err', err.max())
            assert err.max() < bar, (tile, err.max())
        else:
            assert helpers.bits_equal(got, first), tile
    best = ctypes.c_float(0.0)
    hip.check(hip.lib().gpp_mobilenet_block_autotune(ctypes.byref(d), 2, hip.stream_ptr(), ctypes.byref(best)), 'autotune')
    assert d.tile_hint in list(tiles[:count.value]) and best.value > 0


def test_block_image_does_not_depend_on_its_batch():
    d2, keep2, out2, _, _, _ = block_case(32, 64, 3, 13, 18, 2, 'f16x3')
    run_block(d2)
    whole = out2.cpu().numpy()
    xin = keep2[5]
    one_in = xin[2:3].contiguous()
    one_out = torch.zeros((1,) + tuple(out2.shape[1:]), dtype=torch.float32, device='cuda')
    d1 = M.block_desc(C.FMap(one_in, 1, 13, 18, 32, pitch=40), C.FMap(one_out, 1, out2.shape[1], out2.shape[2], 64), keep2[0], keep2[1],
                      keep2[2], keep2[3], keep2[4], 2, 'f16x3')
    run_block(d1)
    assert helpers.bits_equal(one_out.cpu().numpy()[0], whole[2])


def test_block_refuses_what_it_does_not_do():
    d, keep, _, _, _, _ = block_case(32, 64, 1, 6, 6, 1, 'f32')
    lib = hip.lib()
    for field, value, rc in (('dtype', hip.GPP_BF16, -4), ('dtype', hip.GPP_F16, -4), ('stride', 3, -4), ('C_in', 30, -1), ('tile_hint', 5, -1),
                             ('weight_rows', 64, -1), ('in_pitch', 16, -1)):
        old = getattr(d, field)
        setattr(d, field, value)
        assert lib.gpp_mobilenet_block(ctypes.byref(d), hip.stream_ptr()) == rc, field
        setattr(d, field, old)
    run_block(d)


@pytest.mark.parametrize('hw', [(32, 48), (33, 47)])
@pytest.mark.parametrize('cout', [8, 32])
def test_stem_bit_exact(hw, cout):
    """ 27 taps in (dy, dx, input channel) order, float32 multiply then add, + bias, clamp: the NumPy loop gives the same bits """
    H, Wd = hw
    B, pitch = 2, cout + 4
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - MEAN
    w = (rng.standard_normal((27, cout)) * 0.02).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.5).astype(np.float32)
    Ho, Wo = M.out_size(H, 2), M.out_size(Wd, 2)
    xin, wt, bt = torch.as_tensor(x).cuda(), torch.as_tensor(w).cuda(), torch.as_tensor(b).cuda()
    out = torch.full((B, Ho, Wo, pitch), 7.0, device='cuda')
    hip.check(hip.lib().gpp_mobilenet_stem(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(wt.data_ptr()), ctypes.c_void_p(bt.data_ptr()),
                                           ctypes.c_void_p(out.data_ptr()), B, H, Wd, cout, pitch, hip.stream_ptr()), 'gpp_mobilenet_stem')
    v = None
    for t9, tap in enumerate(padded_taps(x, 2, Ho, Wo)):
        for ci in range(3):
            prod = tap[..., ci:ci + 1] * w[t9 * 3 + ci][None, None, None, :]
            v = prod if v is None else v + prod
    want = np.minimum(np.maximum(v + b, np.float32(0)), np.float32(6))
    assert want.dtype == np.float32 and (want == 6).any() and (want == 0).any()
    got = out.cpu().numpy()
    assert helpers.bits_equal(got[..., :cout], want) and (got[..., cout:] == 7.0).all()


def frames(B, H, Wd, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - MEAN


def reference(weights, img, P_inv, planes, oracle_lib, backbone):
    f = MO.forward(weights, img, backbone, precision='f64')
    det, aidx = MO.detect(f)
    kp, kpl, res, idx = helpers.c_oracle_poll(oracle_lib, det[0], det[1], det[4], P_inv, planes)
    return f, list(det) + [kp, kpl, res], aidx, idx


def inputs(B):
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))


BACKBONE = 'mobilenet224_1.0'


@pytest.fixture(scope='module')
def reduced(oracle_lib):
    B, H, Wd = 2, 160, 512
    weights = W.synthetic_weights(BACKBONE, 1234)
    img = frames(B, H, Wd)
    P_inv, planes = inputs(B)
    return (B, H, Wd, weights, img, P_inv, planes) + reference(weights, img, P_inv, planes, oracle_lib, BACKBONE)


def check_against_oracle(model, plan, out, f, ref, aidx, idx, pair):
    B = out[0].shape[0]
    assert plan.n_anchors == f['classification_logits'].shape[1]
    for name in ('C3', 'C4', 'C5'):
        got = plan.features[name].read().cpu().numpy()
        assert got.shape == f[name].shape
        assert got.min() >= 0.0 and got.max() <= 6.0                        # what the FPN reads are the post-ReLU6 maps
        assert np.abs(got - f[name]).max() <= 1e-3 * (np.abs(f[name]).max() + 1.0), name
    cls = plan.cls_logits.cpu().numpy().reshape(B, -1, 8)
    assert np.abs(cls - f['classification_logits']).max() < 1e-3
    led = ledger.parity_ledger(ref, aidx, idx, out, plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=pair), led


@pytest.mark.parametrize('dtype', ['f32', 'f16x3'])
def test_mobilenet224_end_to_end(reduced, dtype, monkeypatch):
    B, H, Wd, weights, img, P_inv, planes, f, ref, aidx, idx = reduced
    if dtype == 'f16x3':
        monkeypatch.setenv('GPP_TUNE_RANDOM', '5')      # random tiles of every layer: the result may not depend on them
    model = models.load_model(weights, backbone_name=BACKBONE, dtype=dtype)
    assert model.backbone_name == BACKBONE
    out = model.predict_on_batch([img, P_inv, planes])
    assert len(out) == 8
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    assert sum(1 for kind, _, _, _, _ in plan.ops if kind == 34) == 13       # one launch per depthwise-separable block
    check_against_oracle(model, plan, out, f, ref, aidx, idx, pair=dtype != 'f32')
    # batch independence: image 1 alone gives the bytes it gets inside the batch of 2
    one = model.predict_on_batch([img[1:], P_inv[1:], planes[1:]])
    for a, b in zip(one, out):
        assert helpers.bits_equal(a[0], b[1])
    model.capture(plan)                                   # the plan captures into a graph and replays the same bytes
    stage = model.stage_inputs([img, P_inv, planes])
    model.run_plan(stage)
    again = model.fetch(stage)
    for a, b in zip(again, out):
        assert helpers.bits_equal(a, b)


def test_mobilenet224_latency_plan(reduced):
    B, H, Wd, weights, img, P_inv, planes, f, ref, aidx, idx = reduced
    model = models.load_model(weights, backbone_name=BACKBONE, dtype='f16x3', plan='latency')
    out = model.predict_on_batch([img, P_inv, planes])
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    led = ledger.parity_ledger(ref, aidx, idx, out, plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=True), led


def test_mobilenet224_pose_rows(reduced):
    B, H, Wd, weights, img, P_inv, planes = reduced[:7]
    model = models.load_model(weights, backbone_name=BACKBONE, dtype='f16x3', pose=True)
    rows, counts = model.predict_poses_on_batch([img, P_inv, planes], 1.0, (H, Wd, 3))
    assert rows.shape == (B, 100, 36) and counts.shape == (B,)


def test_mobilenet_quarter_width_end_to_end(oracle_lib):
    """ alpha 0.25: C_in 8 / 16 (zero-filled K-chunks), C_out 16 .. 256 """
    backbone = 'mobilenet128_0.25'
    B, H, Wd = 1, 128, 384
    weights = W.synthetic_weights(backbone, 1234)
    img = frames(B, H, Wd, 2)
    P_inv, planes = inputs(B)
    f, ref, aidx, idx = reference(weights, img, P_inv, planes, oracle_lib, backbone)
    model = models.load_model(weights, backbone_name=backbone, dtype='f16x3')
    out = model.predict_on_batch([img, P_inv, planes])
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    check_against_oracle(model, plan, out, f, ref, aidx, idx, pair=True)


@pytest.mark.slow
@pytest.mark.parametrize('backbone', ['mobilenet192_0.5', 'mobilenet160_0.75'])
def test_other_widths_end_to_end(backbone, oracle_lib):
    B, H, Wd = 1, 128, 384
    weights = W.synthetic_weights(backbone, 1234)
    img = frames(B, H, Wd, 2)
    P_inv, planes = inputs(B)
    f, ref, aidx, idx = reference(weights, img, P_inv, planes, oracle_lib, backbone)
    model = models.load_model(weights, backbone_name=backbone, dtype='f16x3')
    out = model.predict_on_batch([img, P_inv, planes])
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    check_against_oracle(model, plan, out, f, ref, aidx, idx, pair=True)


@pytest.mark.slow
def test_mobilenet224_full_size_f16x3_against_f32():
    B, H, Wd = 1, 402, 1333
    weights = W.synthetic_weights(BACKBONE, 1234)
    img = frames(B, H, Wd, 1)
    P_inv, planes = inputs(B)
    o32 = models.load_model(weights, backbone_name=BACKBONE, dtype='f32')
    out32 = o32.predict_on_batch([img, P_inv, planes])
    p32 = o32.plan_for(B, H, Wd, planes.shape[1], True)
    o16 = models.load_model(weights, backbone_name=BACKBONE, dtype='f16x3')
    out16 = o16.predict_on_batch([img, P_inv, planes])
    p16 = o16.plan_for(B, H, Wd, planes.shape[1], True)
    assert p16.n_anchors == 137256
    led = ledger.parity_ledger(out32, p32.anchor_index.cpu().numpy(), p32.best_index.cpu().numpy(),
                               out16, p16.anchor_index.cpu().numpy(), p16.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=True), led
