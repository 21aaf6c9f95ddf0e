"""
gpp_bottleneck_block_proj (csrc/conv_block_impl.h, the PROJ form): res2a -- branch2a 1x1, branch1 1x1 (the projection shortcut), branch2b 3x3,
branch2c 1x1 + shortcut + ReLU -- in ONE launch that computes the shortcut from the input rows branch2a stages in LDS; the shortcut never
becomes a map.  The bar is the bytes of the four separate launches (gpp_conv2d_igemm x 4), range events included, with every map the fused
launch must not touch poisoned; the block's input pre-split (as the other fused blocks read theirs) or float32 (pool1's map, what a plan
hands res2a).  Plan level: GPP_FUSE_BLOCK_INPROJ on against off, every output byte.
"""
import ctypes

import numpy as np
import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from keras_retinanet_3D.utils import synthetic

pytestmark = pytest.mark.gpu

UNSUPPORTED, BAD_ARG = -4, -1


def make_block(B, H, W, dtype, xin='split', seed=0, x_scale=1.0, proj_scale=1.0, cin=64, cmid=64):
    """ the four layers of a stride-1 projection bottleneck over fresh maps, a weight scale per output channel (as tests/test_block_gpu.py) """
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(1000 * H + W + B + seed)
    cout = 4 * cmid
    x = torch.randn((B, H, W, cin), generator=g) * x_scale
    ks = [torch.randn((1, 1, cin, cmid), generator=g) * (2.0 / cin) ** 0.5,
          torch.randn((3, 3, cmid, cmid), generator=g) * (2.0 / (9 * cmid)) ** 0.5,
          torch.randn((1, 1, cmid, cout), generator=g) * (1.0 / cmid) ** 0.5,
          torch.randn((1, 1, cin, cout), generator=g) * (1.0 / cin) ** 0.5 * proj_scale]
    ks = [k * torch.pow(2.0, torch.randint(-3, 4, (k.shape[3],), generator=g).float())[None, None, None, :] for k in ks]
    bs = [torch.randn((k.shape[3],), generator=g) * 0.1 for k in ks]

    def fmap(c, split=True):
        return C.FMap.empty(B, H, W, c, torch.float32, dev, split=split, half=dtype)
    x_map = fmap(cin, split=(xin == 'split'))
    x_map.write(x.to(dev))
    a, bmap, sc = fmap(cmid), fmap(cmid), fmap(cout)
    ws = [C.pack_weight(k.numpy(), dtype, dev) for k in ks]
    ss = [C.out_scale_of(k.numpy(), dev) if dtype == 'f16x3' else None for k in ks]
    bd = [b.to(dev) for b in bs]

    def descs(y, fused):
        d1 = C.conv_desc([x_map], [a], ws[0], bd[0], 1, 1, cin, cmid, relu=True, dtype=dtype, out_scale=ss[0])
        d2 = C.conv_desc([a], [bmap], ws[1], bd[1], 3, 3, cmid, cmid, pad=(1, 1), relu=True, dtype=dtype, out_scale=ss[1])
        d3 = C.conv_desc([bmap], [y], ws[2], bd[2], 1, 1, cmid, cout, relu=True, residuals=None if fused else [sc], dtype=dtype, out_scale=ss[2])
        dp = C.conv_desc([x_map], [sc], ws[3], bd[3], 1, 1, cin, cout, dtype=dtype, out_scale=ss[3])
        return d1, d2, d3, dp
    return dict(x=x_map, a=a, b=bmap, sc=sc, fmap=fmap, descs=descs, keep=(ws, ss, bd), cout=cout)


def run_separate(blk, y):
    d1, d2, d3, dp = blk['descs'](y, False)
    for d in (d1, dp, d2, d3):
        C.run_conv(d)


def run_fused(d1, d2, d3, dp, tile=0):
    return hip.lib().gpp_bottleneck_block_proj(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3), ctypes.byref(dp), tile, hip.stream_ptr())


def poison(*maps):
    for m in maps:
        m.buf.fill_(float('nan'))


SHAPES = [(2, 25, 31), (3, 9, 40), (1, 7, 5), (1, 1, 1), (2, 8, 14), (2, 16, 28), (1, 17, 29), (1, 101, 67)]


@pytest.mark.parametrize('xin', ['split', 'f32'])
@pytest.mark.parametrize('dtype', ['f16x3', 'bf16x3'])
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_projection_block_in_one_launch_gives_the_bytes_of_its_four_layers(B, H, W, dtype, xin):
    blk = make_block(B, H, W, dtype, xin=xin)
    y_sep, y = blk['fmap'](blk['cout']), blk['fmap'](blk['cout'])
    run_separate(blk, y_sep)
    want = y_sep.buf.clone()
    assert torch.isfinite(y_sep.read()).all() and float(y_sep.read().abs().max()) > 0
    for tile in (0, 814):                                      # every tile code the C = 64 form accepts
        poison(blk['a'], blk['b'], blk['sc'], y)
        hip.check(run_fused(*blk['descs'](y, True), tile=tile), 'gpp_bottleneck_block_proj')
        assert torch.equal(y.buf.view(torch.int32), want.view(torch.int32))
        assert torch.isnan(blk['a'].buf).all() and torch.isnan(blk['b'].buf).all() and torch.isnan(blk['sc'].buf).all()


@pytest.mark.parametrize('xin', ['split', 'f32'])
@pytest.mark.parametrize('case', ['input', 'branch1'])
def test_block_counts_the_range_events_its_four_layers_count(case, xin):
    """ GPP_F16X3: values beyond the half range are clamped and counted once per stored group, for the pixels a tile owns.  'input': x itself is
    large (every layer overflows); 'branch1': only the projection's weights are (a and b stay in range, the shortcut does not) """
    blk = make_block(1, 20, 30, 'f16x3', xin=xin, x_scale=3.0e4) if case == 'input' else make_block(1, 20, 30, 'f16x3', xin=xin, proj_scale=2.0 ** 17)
    n = ctypes.c_uint64(0)
    y_sep, y = blk['fmap'](blk['cout']), blk['fmap'](blk['cout'])
    d1, d2, d3, dp = blk['descs'](y_sep, False)
    hip.check(hip.lib().gpp_x3_range_events(ctypes.byref(n), 1), 'reset')
    C.run_conv(dp)
    hip.check(hip.lib().gpp_x3_range_events(ctypes.byref(n), 1), 'read')
    of_branch1 = int(n.value)
    assert of_branch1 > 0
    for d in (d1, d2):
        C.run_conv(d)
    hip.check(hip.lib().gpp_x3_range_events(ctypes.byref(n), 1), 'read')
    assert case == 'input' or int(n.value) == 0
    separate = of_branch1 + int(n.value)
    C.run_conv(d3)
    hip.check(hip.lib().gpp_x3_range_events(ctypes.byref(n), 1), 'read')
    separate += int(n.value)
    poison(blk['a'], blk['b'], blk['sc'], y)
    hip.check(run_fused(*blk['descs'](y, True)), 'gpp_bottleneck_block_proj')
    hip.check(hip.lib().gpp_x3_range_events(ctypes.byref(n), 1), 'read')
    assert int(n.value) == separate
    assert torch.equal(y.buf.view(torch.int32), y_sep.buf.view(torch.int32))


def test_block_proj_arguments_are_validated():
    """ every refusal comes before anything is launched: the poisoned output stays poisoned """
    dev = torch.device('cuda')
    blk = make_block(1, 9, 11, 'f16x3')
    ws, ss, bd = blk['keep']
    y = blk['fmap'](256)
    d1, d2, d3, dp = blk['descs'](y, True)
    lib, st = hip.lib(), hip.stream_ptr()

    def copy(d, **fields):
        q = hip.ConvDesc.from_buffer_copy(d)
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    def conv(inp, out, i, cin, cout, **kw):
        return C.conv_desc([inp], [out], ws[i], bd[i], 1, 1, cin, cout, dtype='f16x3', out_scale=ss[i], **kw)
    refused = []
    # another type: the same block in float32
    k32 =[C.pack_weight(torch.zeros(s).numpy(), 'f32', dev) for s in ((1, 1, 64, 64), (3, 3, 64, 64), (1, 1, 64, 256), (1, 1, 64, 256))]
    plain = [C.FMap.empty(1, 9, 11, c, torch.float32, dev) for c in (64, 64, 64, 256, 256)]
    g1 = C.conv_desc([plain[0]], [plain[1]], k32[0], bd[0], 1, 1, 64, 64, relu=True, dtype='f32')
    g2 = C.conv_desc([plain[1]], [plain[2]], k32[1], bd[1], 3, 3, 64, 64, pad=(1, 1), relu=True, dtype='f32')
    g3 = C.conv_desc([plain[2]], [plain[3]], k32[2], bd[2], 1, 1, 64, 256, relu=True, dtype='f32')
    gp = C.conv_desc([plain[0]], [plain[4]], k32[3], bd[3], 1, 1, 64, 256, dtype='f32')
    refused.append(('float32 layers', (g1, g2, g3, gp)))
    # maps that are not pre-split: the output, the intermediate map, the shortcut's
    y_plain, a_plain = C.FMap.empty(1, 9, 11, 256, torch.float32, dev), C.FMap.empty(1, 9, 11, 64, torch.float32, dev)
    refused.append(('float32 output map', (d1, d2, conv(blk['b'], y_plain, 2, 64, 256, relu=True), dp)))
    refused.append(('float32 a map', (conv(blk['x'], a_plain, 0, 64, 64, relu=True), d2, d3, dp)))
    refused.append(('float32 shortcut map', (d1, d2, d3, conv(blk['x'], y_plain, 3, 64, 256))))
    # C_mid != 64
    wide = make_block(1, 9, 11, 'f16x3', cin=64, cmid=128)
    refused.append(('C = 128', wide['descs'](wide['fmap'](512), True)))
    deep = make_block(1, 9, 11, 'f16x3', cin=128, cmid=64)               # res2a's shape only: C_in = 64
    refused.append(('C_in = 128', deep['descs'](y, True)))
    # a stride on either 1x1 (the maps keep their size: the stride alone is the difference)
    refused.append(('stride 2 on branch2a', (copy(d1, stride=2), d2, d3, dp)))
    refused.append(('stride 2 on branch1', (d1, d2, d3, copy(dp, stride=2))))
    # branch1 reads another map / pitch / offsets than branch2a
    other = blk['fmap'](64)
    other.buf.zero_()
    refused.append(('another input map', (d1, d2, d3, conv(other, blk['sc'], 3, 64, 256))))
    refused.append(('another input pitch', (d1, d2, d3, copy(dp, in_pitch=128))))
    q = copy(dp)
    q.groups[0].in_off = 32
    refused.append(('another input offset', (d1, d2, d3, q)))
    # C_out of branch1 and branch2c differ
    refused.append(('branch1 C_out', (d1, d2, d3, copy(dp, C_out=128))))
    # branch1 with a residual, a ReLU, lists or a guard
    refused.append(('branch1 residual', (d1, d2, d3, conv(blk['x'], blk['sc'], 3, 64, 256, residuals=[y]))))
    refused.append(('branch1 relu', (d1, d2, d3, copy(dp, relu=1))))
    flag = torch.zeros((4,), dtype=torch.int32, device=dev)
    refused.append(('branch1 guard', (d1, d2, d3, copy(dp, guard=flag.data_ptr()))))
    refused.append(('branch1 lists', (d1, d2, d3, copy(dp, gather_rows=flag.data_ptr(), gather_counts=flag.data_ptr()))))
    # branch2c with a shortcut map: the shortcut is not a map
    refused.append(('branch2c residual', blk['descs'](y, False)))
    for what, ds in refused:
        poison(y, y_plain, *plain[1:])
        assert run_fused(*ds) == UNSUPPORTED, what
        torch.cuda.synchronize()
        assert torch.isnan(y.buf).all() and torch.isnan(y_plain.buf).all() and all(torch.isnan(p.buf).all() for p in plain[1:]), what
    poison(y)
    assert run_fused(d1, d2, d3, dp, 999) == BAD_ARG                      # not a tile code
    assert lib.gpp_bottleneck_block_proj(ctypes.byref(d1), ctypes.byref(d2), ctypes.byref(d3), None, 0, st) == BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(y.buf).all()
    assert run_fused(d1, d2, d3, dp) == 0                                 # ... and the block as it is runs
    torch.cuda.synchronize()
    assert torch.isfinite(y.read()).all()


def test_plan_with_the_fused_projection_block_gives_the_bytes_of_the_plan_without(monkeypatch):
    """ (2, 224, 352), f16x3: res2a as one launch against its three launches -- the eight outputs, the three head tensors, C2 .. C5, the flops,
    the range events and the stream ordering """
    B, H, Wd = 2, 224, 352
    monkeypatch.setenv('GPP_FUSE_INPROJ_MIN_ROUNDS', '0')
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(B, H, Wd, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    inputs = [img, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))]
    got = {}
    for switch in ('1', '0'):
        monkeypatch.setenv('GPP_FUSE_BLOCK_INPROJ', switch)
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
        out = model.predict_on_batch(inputs)
        plan = model.plan_for(B, H, Wd, planes.shape[0], True)
        torch.cuda.synchronize()
        names = [op[3] for op in plan.ops]
        got[switch] = dict(out=[np.array(o) for o in out], names=names, flops=plan.flops, order=plan.check_stream_ordering(),
                           events=int(plan.range_slot.cpu()[0]),
                           heads=[t.cpu().numpy().copy() for t in (plan.cls_logits, plan.regression, plan.regression_dim)],
                           feats=[plan.features[k].buf.cpu().numpy().copy() for k in ('C2', 'C3', 'C4', 'C5')])
    on, off = got['1'], got['0']
    assert 'res2a_branch1' not in on['names'] and 'res2a_branch2a' not in on['names'] and on['names'].count('res2a_branch2a+2b+2c') == 2
    assert off['names'].count('res2a_branch1') == 2 and off['names'].count('res2a_branch2a') == 2
    assert on['order'] == [] and off['order'] == []
    assert on['flops'] == off['flops'] and on['events'] == off['events']
    assert len(on['out']) == 8
    for a, b in zip(on['out'] + on['heads'] + on['feats'], off['out'] + off['heads'] + off['feats']):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
