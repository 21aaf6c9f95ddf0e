"""
MobileNet backbones (reference models/mobilenet.py), the parts that need no GPU: the Keras layer inventory and its parameter count, the
dispatch of backbone names, the feature / anchor shapes, the oracle's padding rule and tap order against a loop-written NumPy block, the
synthetic draw and its calibration, weight files with 'depthwise_kernel', and the race check of CPU-built plans.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import mobilenet_oracle as MO
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import retinanet as R
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import anchors as A
from keras_retinanet_3D.utils import ledger

MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def test_inventory_matches_keras():
    """ 3 228 864: Keras' published include_top=False total of MobileNet 1.0 (BatchNormalization: 4 per channel) """
    bb = 'mobilenet224_1.0'
    assert W.backbone_parameter_count(bb) == 3228864
    assert W.backbone_parameter_count('mobilenet128_1.0') == 3228864          # the rows do not change the graph
    layers = W.mobilenet_layers(bb)
    assert layers[0] == ('conv', 'conv1', (3, 3, 3, 32)) and layers[-1] == ('bn', 'conv_pw_13_bn', (1024,))
    assert layers[2] == ('dw', 'conv_dw_1', (3, 3, 32, 1))
    assert sum(1 for kind, _, _ in layers if kind == 'dw') == 13 and sum(1 for kind, _, _ in layers if kind == 'conv') == 14
    assert [s for _, _, _, s in W.mobilenet_blocks(bb)] == [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]
    W.validate_weights(W.synthetic_weights(bb, 3), bb)
    with pytest.raises(ValueError, match='conv_dw_1/depthwise_kernel'):
        bad = W.synthetic_weights(bb, 3)
        del bad['conv_dw_1/depthwise_kernel']
        W.validate_weights(bad, bb)
    assert W.bn_epsilon(bb) == 1e-3 and W.bn_epsilon('resnet50') == 1e-5
    assert W.fpn_layers() == W.fpn_layers('resnet50')                         # the ResNet table, unchanged


@pytest.mark.parametrize('alpha,c0,widths', [('0.25', 8, (32, 64, 128, 256)), ('0.5', 16, (64, 128, 256, 512)),
                                             ('0.75', 24, (96, 192, 384, 768)), ('1.0', 32, (128, 256, 512, 1024))])
def test_widths_follow_alpha(alpha, c0, widths):
    bb = 'mobilenet192_' + alpha
    assert W.mobilenet_filters(bb)[0] == c0 and tuple(W.mobilenet_widths(bb)) == widths
    fpn = {name: cin for name, _, cin, _, _ in W.fpn_layers(bb)}
    assert (fpn['C3_reduced'], fpn['C4_reduced'], fpn['C5_reduced'], fpn['P6']) == widths[1:] + (widths[3],)
    assert all(w % 32 == 0 for w in widths[1:])                               # the FPN convs take them as they are


def test_backbone_dispatch():
    assert models.backbone('mobilenet224_1.0').backbone == 'mobilenet224_1.0'
    assert models.backbone('mobilenet128_0.25').backbone == 'mobilenet128_0.25'
    with pytest.raises(ValueError, match='allowed backbones'):
        models.backbone('mobilenet100_1.0')
    with pytest.raises(ValueError, match=r'0\.25, 0\.5, 0\.75, 1\.0'):
        models.backbone('mobilenet224_0.3')
    with pytest.raises(NotImplementedError, match='multiplier is missing'):
        models.backbone('mobilenet224')
    assert W.is_mobilenet('mobilenet224_1.0') and not W.is_mobilenet('mobilenet224') and not W.is_mobilenet('mobilenet224_0.3')
    assert not W.is_mobilenet('resnet50') and not W.is_densenet('mobilenet224_1.0')


@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
def test_16_bit_storage_is_refused(dtype):
    with pytest.raises(ValueError, match="'f32', 'f16x3' or 'bf16x3'"):
        R.RetinaNet3D(W.synthetic_weights('mobilenet224_0.25', 1), backbone_name='mobilenet224_0.25', dtype=dtype)


def test_anchors_at_402x1333():
    """ every stride-2 layer gives ceil(n / 2): the ResNet pyramid """
    assert A.pyramid_shapes((402, 1333))[:3] == [(51, 167), (26, 84), (13, 42)]
    assert len(A.anchors_for_image((402, 1333))) == 137256


@pytest.mark.parametrize('hw', [(64, 96), (67, 101)])
def test_oracle_shapes_match_the_helper(hw):
    img = np.random.default_rng(1).integers(0, 256, size=(1,) + hw + (3,)).astype(np.float32) - MEAN
    bb = 'mobilenet224_0.5'
    out = MO.forward(W.synthetic_weights(bb, 5), img, bb)
    shapes = [tuple(s) for s in A.pyramid_shapes(hw)]
    assert [tuple(out[k].shape[1:3]) for k in ('C3', 'C4', 'C5')] == shapes[:3]
    assert [tuple(out[k].shape[1:3]) for k in ('P3', 'P4', 'P5', 'P6', 'P7')] == shapes
    assert out['classification_logits'].shape[1] == len(A.anchors_for_image(hw))
    assert [out[k].shape[3] for k in ('C2', 'C3', 'C4', 'C5')] == W.mobilenet_widths(bb)
    assert all(out[k].min() >= 0 and out[k].max() <= 6 for k in ('C3', 'C4', 'C5'))


def loop_block(x, kd, bn_d, kp, bn_p, stride, eps=1e-3):
    """ one depthwise-separable block written as loops, float64, NHWC, one image: symmetric pad 1, window origin o * stride - 1, taps in
    (dy, dx) order -- the rule and the order csrc/mobilenet.hip documents; BN literal """
    H, Wd, Cc = x.shape
    Ho, Wo = (H - 1) // stride + 1, (Wd - 1) // stride + 1
    mid = np.zeros((Ho, Wo, Cc))
    for oy in range(Ho):
        for ox in range(Wo):
            for c in range(Cc):
                v = 0.0
                for dy in range(3):
                    for dx in range(3):
                        iy, ix = oy * stride - 1 + dy, ox * stride - 1 + dx
                        if 0 <= iy < H and 0 <= ix < Wd:
                            v += x[iy, ix, c] * kd[dy, dx, c, 0]
                g, b, m, var = bn_d
                mid[oy, ox, c] = min(max((v - m[c]) / np.sqrt(var[c] + eps) * g[c] + b[c], 0.0), 6.0)
    out = np.zeros((Ho, Wo, kp.shape[3]))
    g, b, m, var = bn_p
    for oy in range(Ho):
        for ox in range(Wo):
            for n in range(kp.shape[3]):
                v = 0.0
                for c in range(Cc):
                    v += mid[oy, ox, c] * kp[0, 0, c, n]
                out[oy, ox, n] = min(max((v - m[n]) / np.sqrt(var[n] + eps) * g[n] + b[n], 0.0), 6.0)
    return out


@pytest.mark.parametrize('hw', [(6, 8), (7, 9)])
@pytest.mark.parametrize('stride', [1, 2])
def test_oracle_block_against_numpy_loops(hw, stride):
    """ pins the padding rule: at stride 2 on an even side TF's 'same' window would start at 2 o, this one at 2 o - 1 """
    rng = np.random.default_rng(4)
    cin, cout = 4, 8
    x = np.clip(rng.standard_normal(hw + (cin,)) * 2, 0, 6)
    w = {'conv_dw_1/depthwise_kernel': rng.standard_normal((3, 3, cin, 1)), 'conv_pw_1/kernel': rng.standard_normal((1, 1, cin, cout))}
    for name, c in (('conv_dw_1_bn', cin), ('conv_pw_1_bn', cout)):
        w[name + '/gamma'], w[name + '/beta'] = 1 + 0.3 * rng.standard_normal(c), rng.standard_normal(c)
        w[name + '/moving_mean'], w[name + '/moving_variance'] = rng.standard_normal(c), 0.5 + rng.random(c)
    net = MO.MobileNetNet(w, 'mobilenet224_1.0', 'f64')
    with torch.no_grad():
        got = net.depthwise_block(torch.as_tensor(x).permute(2, 0, 1)[None], 1, stride)[0].permute(1, 2, 0).numpy()
    bn = lambda n: tuple(w[n + '/' + p] for p in ('gamma', 'beta', 'moving_mean', 'moving_variance'))        # noqa: E731
    want = loop_block(x, w['conv_dw_1/depthwise_kernel'], bn('conv_dw_1_bn'), w['conv_pw_1/kernel'], bn('conv_pw_1_bn'), stride)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-12
    assert (want == 0).any() and (want == 6).any()
    if stride == 2 and hw[0] % 2 == 0:
        # the TF 'same' window of the same layer (pad 0 before, 1 after) gives another map: the test would see the wrong rule
        shifted = loop_block(np.pad(x, ((0, 1), (0, 1), (0, 0)))[1:, 1:], w['conv_dw_1/depthwise_kernel'], bn('conv_dw_1_bn'),
                             w['conv_pw_1/kernel'], bn('conv_pw_1_bn'), stride)
        assert shifted.shape != want.shape or np.abs(shifted - want).max() > 1e-3


def test_synthetic_draw_is_seeded_and_trained_family_rescales():
    bb = 'mobilenet224_0.5'
    a, b = W.synthetic_weights(bb, 7), W.synthetic_weights(bb, 7)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a['conv1/kernel'], W.synthetic_weights(bb, 8)['conv1/kernel'])
    t = W.synthetic_weights(bb, 7, 'trained')
    assert set(t) == set(a)
    g = np.abs(t['conv_pw_5/kernel']).max(axis=(0, 1, 2)) / np.abs(a['conv_pw_5/kernel']).max(axis=(0, 1, 2))
    assert g.max() / g.min() > 30                            # most of two decades between the output channels of one kernel
    assert (t['conv_pw_5_bn/moving_variance'] > 0).all()
    # ... and the function is the base draw's: BatchNormalization carries the matching statistics
    img = np.random.default_rng(2).integers(0, 256, size=(1, 64, 96, 3)).astype(np.float32) - MEAN
    fa, ft = MO.forward(a, img, bb, precision='f64'), MO.forward(t, img, bb, precision='f64')
    assert np.abs(fa['C5'] - ft['C5']).max() < 1e-4 * (np.abs(fa['C5']).max() + 1)


def test_synthetic_calibration():
    """ about 10^3 anchors per 402x1333 noise frame above the 0.05 score threshold (the target of the other draws), float32 oracle.
    ReLU6 saturates: the draw keeps the clamp alive but rare.  Measured with seed 1234: 954 anchors; over the 27 activation maps 0.13 %
    of the values sit at 6 (0.6 % in conv_dw_1, the most saturated map) and 49 % lie strictly between 0 and 6 (the rest are 0). """
    bb = 'mobilenet224_1.0'
    img = np.random.default_rng(0).integers(0, 256, size=(1, 402, 1333, 3)).astype(np.float32) - MEAN
    sat = {}
    out = MO.forward(W.synthetic_weights(bb, 1234), img, bb, saturation=sat)
    assert out['classification_logits'].shape[1] == 137256
    p = 1.0 / (1.0 + np.exp(-out['classification_logits'].reshape(1, -1, 8)))
    n = int((p.max(axis=2) > 0.05).sum())
    at6, inside = np.array([v[0] for v in sat.values()]), np.array([v[1] for v in sat.values()])
    print('anchors above 0.05:', n, 'share at 6: mean', at6.mean(), 'max', at6.max(), 'share inside (0, 6): mean', inside.mean())
    assert 500 <= n <= 2000, n
    assert len(sat) == 27
    assert at6.max() > 1e-3 and at6.max() < 0.05             # some at 6 ...
    assert inside.min() > 0.3                                # ... most of the live ones below it, in every map


@pytest.mark.parametrize('ext', ['h5', 'npz'])
def test_weight_file_round_trip_with_depthwise_kernel(tmp_path, ext):
    bb = 'mobilenet160_0.25'
    w = W.synthetic_weights(bb, 11)
    path = str(tmp_path / ('m.' + ext))
    try:
        W.save_weights(path, w)
    except OSError as exc:         # no HDF5 library on this machine at all
        pytest.skip(str(exc))
    back = W.load_weights(path)
    assert 'conv_dw_1/depthwise_kernel' in back and 'conv_dw_1/kernel' not in back
    assert set(back) == set(w)
    assert all(np.array_equal(back[k], w[k]) for k in w)
    W.validate_weights(back, bb)


def test_float32_oracle_meets_the_bars_on_the_gpu_tests_frames(oracle_lib):
    """ the frames and seed of tests/test_mobilenet_gpu.py: the float32 oracle itself must be inside the ledger bars against the float64
    oracle there (ties at the top-k cut included), or the GPU test would measure the frame, not the kernels """
    import helpers
    from keras_retinanet_3D.utils import synthetic
    bb = 'mobilenet224_1.0'
    weights = W.synthetic_weights(bb, 1234)
    img = np.random.default_rng(0).integers(0, 256, size=(2, 160, 512, 3)).astype(np.float32) - MEAN
    planes = np.tile(synthetic.load_plane_database('100').astype(np.float32)[None], (2, 1, 1))
    P_inv = np.tile(synthetic.synthetic_calibration()[1][None].astype(np.float32), (2, 1, 1))
    sides = []
    for precision in ('f64', 'f32'):
        f = MO.forward(weights, img, bb, precision=precision)
        det, aidx = MO.detect(f)
        kp, kpl, res, idx = helpers.c_oracle_poll(oracle_lib, det[0], det[1], det[4], P_inv, planes)
        sides.append((f, list(det) + [kp, kpl, res], aidx, idx))
    (f64, ref, aidx, idx), (f32, out, aidx32, idx32) = sides
    assert (ref[2] > 0.05).sum() > 20                        # there is something to compare
    led = ledger.parity_ledger(ref, aidx, idx, out, aidx32, idx32)
    assert ledger.meets_reference_bars(led, pair=False), led
    for name in ('C3', 'C4', 'C5'):
        assert np.abs(f32[name] - f64[name]).max() <= 1e-4 * (np.abs(f64[name]).max() + 1.0)


# ---- CPU-built plans (tests/test_plan_cpu.py builds its models the same way), a configuration list of this file's own
PLAN_CONFIGS = [(bb, dt, B) for bb in ('mobilenet224_1.0', 'mobilenet224_0.25') for dt in ('f32', 'f16x3') for B in (1, 2)]


@pytest.fixture(scope='module')
def cpu_model():
    built = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def model_for(bb, dt):
            if (bb, dt) not in built:
                built[(bb, dt)] = models.load_model('synthetic:1234', backbone_name=bb, dtype=dt)
            return built[(bb, dt)]
        yield model_for


@pytest.mark.parametrize('bb,dt,B', PLAN_CONFIGS, ids=lambda v: str(v))
def test_plan_is_race_free_and_every_descriptor_is_accepted(bb, dt, B, cpu_model):
    model = cpu_model(bb, dt)
    assert model.backbone_name == bb
    plan = model.plan_for(B, 96, 160, 100, True)
    assert plan.check_stream_ordering() == []
    kinds = [kind for kind, _, _, _, _ in plan.ops]
    assert kinds[0] == R.OP_MOBILENET_STEM and kinds[1:14] == [R.OP_MOBILENET_BLOCK] * 13
    assert [R.Plan.stage_of(k, n) for k, _, _, n, _ in plan.ops[:14]] == [1] + [2] * 13
    tiles, count = (ctypes.c_int * 16)(), ctypes.c_int(0)
    for kind, _, desc, name, _ in plan.ops:
        if kind == R.OP_MOBILENET_BLOCK:          # host-side validation of the library: every block descriptor is one it accepts
            assert hip.lib().gpp_mobilenet_block_tile_candidates(ctypes.byref(desc), tiles, 16, ctypes.byref(count)) == 0 and count.value >= 4, name
        elif kind == R.OP_CONV:
            assert hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(desc), tiles, 16, ctypes.byref(count)) == 0 and count.value > 0, name
    assert [tuple(plan.features[k].H for k in ('C3', 'C4', 'C5'))] == [(12, 6, 3)]
    with pytest.raises(hip.GppError):
        model.run_plan(plan)
