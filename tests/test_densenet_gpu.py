"""
DenseNet backbones on the GPU: the pre-activation 1x1 conv (gpp_conv2d_preact) against a float64 W . relu(x * s + t) + b, the two pools
bit for bit against NumPy, and densenet121 end to end against the float64 oracle of tests/densenet_oracle.py within the reference bars.
"""
import ctypes

import numpy as np
import pytest
import torch

import densenet_oracle as DO
import helpers
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import ledger, synthetic

pytestmark = pytest.mark.gpu

MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def preact_case(cin, cout, B, H, Wd, dtype, seed=0):
    rng = np.random.default_rng(seed)
    pitch = cin + 32                                     # a channel prefix of a wider map, as the concatenation buffers are read
    x = rng.standard_normal((B, H, Wd, pitch)).astype(np.float32)
    x[..., :8] = 0.0                                     # zero inputs on channels with gamma < 0, shift > 0: relu(shift) must come through
    s = (rng.standard_normal(cin) * 0.7).astype(np.float32)
    t = (rng.standard_normal(cin) * 0.5).astype(np.float32)
    s[:8], t[:8] = -np.abs(s[:8]) - 0.1, np.abs(t[:8]) + 0.1
    k = (rng.standard_normal((1, 1, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    dev = torch.device('cuda')
    xin = torch.as_tensor(x).to(dev)
    out = torch.zeros((B, H, Wd, cout), dtype=torch.float32, device=dev)
    wt, bias = C.pack_weight(k, dtype, dev), torch.as_tensor(b).to(dev)
    fi, fo = C.FMap(xin, B, H, Wd, cin, pitch=pitch), C.FMap(out, B, H, Wd, cout)
    osc = C.out_scale_of(k, dev) if dtype == 'f16x3' else None          # (kept alive with the descriptor: it holds its address)
    d = C.conv_desc([fi], [fo], wt, bias, 1, 1, cin, cout, relu=True, dtype=dtype, out_scale=osc)
    st, tt = torch.as_tensor(s).to(dev), torch.as_tensor(t).to(dev)
    ref = np.maximum(np.maximum(x[..., :cin].astype(np.float64) * s + t, 0.0) @ k[0, 0].astype(np.float64) + b, 0.0)
    return d, (st, tt, xin, out, wt, bias, osc), out, ref


def run_preact(d, keep):
    hip.check(hip.lib().gpp_conv2d_preact(ctypes.byref(d), ctypes.c_void_p(keep[0].data_ptr()), ctypes.c_void_p(keep[1].data_ptr()),
                                          hip.stream_ptr()), 'gpp_conv2d_preact')


@pytest.mark.parametrize('dtype', ['f32', 'f16x3'])
@pytest.mark.parametrize('cin,cout,hw', [(64, 128, (9, 13)), (256, 128, (17, 31)), (1024, 512, (12, 41))])
def test_preact_against_float64_every_tile(dtype, cin, cout, hw):
    d, keep, out, ref = preact_case(cin, cout, 2, hw[0], hw[1], dtype)
    tiles, count = (ctypes.c_int * 16)(), ctypes.c_int(0)
    hip.check(hip.lib().gpp_conv2d_preact_tile_candidates(ctypes.byref(d), tiles, 16, ctypes.byref(count)), 'candidates')
    first = None
    for tile in tiles[:count.value]:
        d.tile_hint = tile
        out.zero_()
        run_preact(d, keep)
        got = out.cpu().numpy()
        if first is None:
            first = got
            err = np.abs(got - ref) / (np.abs(ref) + 1.0)
            assert err.max() < (2e-5 if dtype == 'f16x3' else 1e-5), (tile, err.max())
        else:
            assert helpers.bits_equal(got, first), tile
    # autotune picks one of them
    best = ctypes.c_float(0.0)
    hip.check(hip.lib().gpp_conv2d_preact_autotune(ctypes.byref(d), ctypes.c_void_p(keep[0].data_ptr()), ctypes.c_void_p(keep[1].data_ptr()),
                                                   2, hip.stream_ptr(), ctypes.byref(best)), 'autotune')
    assert d.tile_hint in list(tiles[:count.value]) and best.value > 0


def test_preact_refuses_16_bit_storage():
    d, keep, _, _ = preact_case(64, 64, 1, 4, 4, 'f32')
    d.dtype = hip.GPP_BF16
    rc = hip.lib().gpp_conv2d_preact(ctypes.byref(d), ctypes.c_void_p(keep[0].data_ptr()), ctypes.c_void_p(keep[1].data_ptr()), hip.stream_ptr())
    assert rc == -4                                       # GPP_ERR_UNSUPPORTED


@pytest.mark.parametrize('hw', [(32, 48), (33, 47)])
def test_pools_bit_exact(hw):
    H, Wd = hw
    B, Cc, pitch = 2, 64, 96
    rng = np.random.default_rng(3)
    x = np.maximum(rng.standard_normal((B, H, Wd, Cc)).astype(np.float32), 0)
    xin = torch.as_tensor(x).cuda()
    Ho, Wo = (H - 1) // 2 + 1, (Wd - 1) // 2 + 1
    out = torch.full((B, Ho, Wo, pitch), 7.0, device='cuda')
    hip.check(hip.lib().gpp_maxpool3x3s2_pad_f32(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, H, Wd, Cc, 1, pitch,
                                                 hip.stream_ptr()), 'maxpool')
    xp = np.full((B, H + 2, Wd + 2, Cc), -np.inf, np.float32)
    xp[:, 1:-1, 1:-1] = x
    want = np.max([xp[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2] for dy in range(3) for dx in range(3)], axis=0)
    got = out.cpu().numpy()
    assert helpers.bits_equal(got[..., :Cc], want) and (got[..., Cc:] == 7.0).all()
    Ha, Wa = H // 2, Wd // 2
    out = torch.full((B, Ha, Wa, pitch), 7.0, device='cuda')
    hip.check(hip.lib().gpp_avgpool2x2_f32(ctypes.c_void_p(xin.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, H, Wd, Cc, pitch,
                                           hip.stream_ptr()), 'avgpool')
    v = x[:, :2 * Ha, :2 * Wa]
    want = (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + v[:, 1::2, 0::2]) + v[:, 1::2, 1::2]) * np.float32(0.25)
    got = out.cpu().numpy()
    assert helpers.bits_equal(got[..., :Cc], want) and (got[..., Cc:] == 7.0).all()


def frames(B, H, Wd, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - MEAN


def reference(weights, img, P_inv, planes, oracle_lib, backbone='densenet121'):
    f = DO.forward(weights, img, backbone, precision='f64')
    det, aidx = DO.detect(f)
    kp, kpl, res, idx = helpers.c_oracle_poll(oracle_lib, det[0], det[1], det[4], P_inv, planes)
    return f, list(det) + [kp, kpl, res], aidx, idx


def inputs(B):
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    return np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))


@pytest.fixture(scope='module')
def reduced(oracle_lib):
    B, H, Wd = 2, 160, 512
    weights = W.synthetic_weights('densenet121', 1234)
    img = frames(B, H, Wd)
    P_inv, planes = inputs(B)
    return (B, H, Wd, weights, img, P_inv, planes) + reference(weights, img, P_inv, planes, oracle_lib)


@pytest.mark.parametrize('dtype', ['f32', 'f16x3'])
def test_densenet121_end_to_end(reduced, dtype, monkeypatch):
    B, H, Wd, weights, img, P_inv, planes, f, ref, aidx, idx = reduced
    if dtype == 'f16x3':
        monkeypatch.setenv('GPP_TUNE_RANDOM', '5')      # random tiles of every layer: the result may not depend on them
    model = models.load_model(weights, backbone_name='densenet121', dtype=dtype)
    out = model.predict_on_batch([img, P_inv, planes])
    assert len(out) == 8
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    assert plan.n_anchors == f['classification_logits'].shape[1]
    for name in ('C3', 'C4', 'C5'):
        got = plan.features[name].read().cpu().numpy()
        assert got.shape == f[name].shape
        assert np.abs(got - f[name]).max() <= 1e-3 * (np.abs(f[name]).max() + 1.0), name
    cls = plan.cls_logits.cpu().numpy().reshape(B, -1, 8)
    assert np.abs(cls - f['classification_logits']).max() < 1e-3
    led = ledger.parity_ledger(ref, aidx, idx, out, plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=dtype != 'f32'), led
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


def test_densenet121_latency_plan(reduced):
    B, H, Wd, weights, img, P_inv, planes, f, ref, aidx, idx = reduced
    model = models.load_model(weights, backbone_name='densenet121', dtype='f16x3', plan='latency')
    out = model.predict_on_batch([img, P_inv, planes])
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    led = ledger.parity_ledger(ref, aidx, idx, out, plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=True), led


@pytest.mark.slow
def test_densenet121_full_size_f16x3_against_f32():
    B, H, Wd = 1, 402, 1333
    weights = W.synthetic_weights('densenet121', 1234)
    img = frames(B, H, Wd, 1)
    P_inv, planes = inputs(B)
    o32 = models.load_model(weights, backbone_name='densenet121', dtype='f32')
    out32 = o32.predict_on_batch([img, P_inv, planes])
    p32 = o32.plan_for(B, H, Wd, planes.shape[1], True)
    o16 = models.load_model(weights, backbone_name='densenet121', dtype='f16x3')
    out16 = o16.predict_on_batch([img, P_inv, planes])
    p16 = o16.plan_for(B, H, Wd, planes.shape[1], True)
    assert p16.n_anchors == 132912
    led = ledger.parity_ledger(out32, p32.anchor_index.cpu().numpy(), p32.best_index.cpu().numpy(),
                               out16, p16.anchor_index.cpu().numpy(), p16.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=True), led


@pytest.mark.slow
@pytest.mark.parametrize('backbone', ['densenet169', 'densenet201'])
def test_deeper_densenets_end_to_end(backbone, oracle_lib):
    B, H, Wd = 1, 128, 384
    weights = W.synthetic_weights(backbone, 1234)
    img = frames(B, H, Wd, 2)
    P_inv, planes = inputs(B)
    _, ref, aidx, idx = reference(weights, img, P_inv, planes, oracle_lib, backbone)
    model = models.load_model(weights, backbone_name=backbone, dtype='f16x3')
    out = model.predict_on_batch([img, P_inv, planes])
    plan = model.plan_for(B, H, Wd, planes.shape[1], True)
    led = ledger.parity_ledger(ref, aidx, idx, out, plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy())
    assert ledger.meets_reference_bars(led, pair=True), led
