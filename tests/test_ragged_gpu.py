""" Ragged batches on the GPU: images of one height class -- the same pool1 map, different heights -- in one call.
The criterion is the determinism contract of README.md: an image's bytes depend on (image, weights, dtype, plan mode) only, so every
comparison with the same image run alone is byte for byte, and no case is excluded.  The kernel tests run at the class Hp = 24 x width 160
(heights 93..96); the canvas rows below an image are filled with large garbage, which no kernel may read as data. """
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import image as I
from keras_retinanet_3D.utils import synthetic

pytestmark = pytest.mark.gpu

HP, WD = 24, 160
HEIGHTS = [95, 93, 96, 94]                     # all four heights of the class, shuffled
# the kernel tests also run at Hp = 23 x width 150: there an image's pooled map is not a whole number of wavefronts of the max pool (a
# wavefront spans two images), its conv map is 75 columns (pool pad_left 1) and the class's largest conv map has an odd row count less
CLASSES = [(24, 160), (23, 150)]
KITTI_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
BGR_MEAN = np.array([103.939, 116.779, 123.68], np.float32)


def raw(t):
    """ the bytes of a tensor / array, for bitwise comparisons (NaN == NaN, -0 != 0) """
    a = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(torch.uint8).numpy().tobytes() if isinstance(a, torch.Tensor) else a.tobytes()


def stem_case(seed, hp, wd, big=False, decades=False):
    """ images of the class's four heights (shuffled) x wd, the canvas holding them (garbage below each image), the stem's kernel and bias, the
    heights table """
    g = torch.Generator().manual_seed(seed)
    hs = [4 * hp - 1, 4 * hp - 3, 4 * hp, 4 * hp - 2]
    imgs = [torch.rand((h, wd, 3), generator=g) * 255.0 - 120.0 for h in hs]
    canvas = torch.rand((len(hs), 4 * hp, wd, 3), generator=g) * 2e4 - 1e4
    for b, im in enumerate(imgs):
        canvas[b, :im.shape[0]] = im
    k = torch.randn((7, 7, 3, 64), generator=g) * (40.0 if big else 0.05)
    if decades:
        k = k * torch.pow(10.0, torch.linspace(-2.0, 2.0, 64))[None, None, None, :]
    bias = torch.randn((64,), generator=g) * (1.0 if not decades else 0.1)
    dev = torch.device('cuda')
    return imgs, canvas.to(dev).contiguous(), k, bias.to(dev), torch.tensor(hs, dtype=torch.int32, device=dev)


def shapes_of(h, wd):
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    return ho, wo, (ho + 1) // 2, (wo + 1) // 2


def check(rc):
    hip.check(rc)


def new(shape, tdt, fill=float('nan')):
    return torch.full(shape, fill, dtype=tdt, device='cuda')


def counter():
    return torch.zeros((1,), dtype=torch.int64, device='cuda')


# ---------------------------------------------------------------------------------------------------- the three dtype families
def run_family(family, dt, tdt, weight, bias, x, B, H, heights, rc_slot):
    """ (conv map of the unfused form, pooled map of the unfused form, pooled map of the fused form or None) of one call: uniform when
    heights is None (x = (B, H, WD, 3)), else ragged (x = the canvas, H = 4 HP) """
    lib, st = hip.lib(), hip.stream_ptr()
    WD = int(x.shape[2])
    ho, wo, hp, wp = shapes_of(H, WD)
    HP = hp
    conv, pool, fused = new((B, ho, wo, 64), tdt), new((B, hp, wp, 64), tdt), None
    p = hip.ptr
    if family == 'f32':
        if heights is None:
            check(lib.gpp_stem_conv7x7_bn_relu(p(x), p(weight), p(bias), p(conv), dt, B, H, WD, st))
        else:
            check(lib.gpp_stem_conv7x7_bn_relu_ragged(p(x), p(weight), p(bias), p(conv), dt, B, H, WD, HP, p(heights), st))
    elif family == 'f16':
        fused = new((B, hp, wp, 64), tdt)
        if heights is None:
            check(lib.gpp_stem_conv7x7_bn_relu_mfma(p(x), p(weight), p(bias), p(conv), dt, B, H, WD, st))
            check(lib.gpp_stem_pool_fused_mfma(p(x), p(weight), p(bias), p(fused), dt, B, H, WD, st))
        else:
            check(lib.gpp_stem_conv7x7_bn_relu_mfma_ragged(p(x), p(weight), p(bias), p(conv), dt, B, H, WD, HP, p(heights), st))
            check(lib.gpp_stem_pool_fused_mfma_ragged(p(x), p(weight), p(bias), p(fused), dt, B, H, WD, HP, p(heights), st))
    else:
        fused = new((B, hp, wp, 64), tdt)
        if heights is None:
            check(lib.gpp_stem_conv7x7_bn_relu_x3_rc(p(x), p(weight), p(bias), p(conv), B, H, WD, p(rc_slot[0]), st))
            check(lib.gpp_stem_pool_fused_x3(p(x), p(weight), p(bias), p(fused), B, H, WD, p(rc_slot[1]), st))
        else:
            check(lib.gpp_stem_conv7x7_bn_relu_x3_rc_ragged(p(x), p(weight), p(bias), p(conv), B, H, WD, HP, p(heights), p(rc_slot[0]), st))
            check(lib.gpp_stem_pool_fused_x3_ragged(p(x), p(weight), p(bias), p(fused), B, H, WD, HP, p(heights), p(rc_slot[1]), st))
    if heights is None:
        check(lib.gpp_maxpool3x3s2_same(p(conv), p(pool), dt if family != 'f16x3' else hip.GPP_F32, B, ho, wo, 64, st))
    else:
        check(lib.gpp_maxpool3x3s2_same_ragged(p(conv), p(pool), dt if family != 'f16x3' else hip.GPP_F32, B, ho, wo, 64, HP, p(heights), st))
    torch.cuda.synchronize()
    return conv, pool, fused


@pytest.mark.parametrize('hp,wd', CLASSES)
@pytest.mark.parametrize('family', ['f32', 'f16', 'f16x3'])
def test_every_ragged_stem_form_equals_the_uniform_function_per_image(family, hp, wd):
    """ a batch holding all four heights of the class, shuffled: the pooled map of image b (unfused and fused form) and the rows of its conv map
    are the uniform functions' on image b alone, byte for byte; conv rows past the image are not touched; the f16x3 counters (weights that
    drive part of the map beyond 65504) equal the sum of the per-image counts """
    imgs, canvas, k, bias, heights = stem_case(11, hp, wd, big=family == 'f16x3')
    dev = canvas.device
    variants = {'f32': [(hip.GPP_F32, torch.float32)], 'f16': [(hip.GPP_F16, torch.float16), (hip.GPP_BF16, torch.bfloat16)],
                'f16x3': [(hip.GPP_F16X3, torch.float32)]}[family]
    weight = {'f32': lambda: k.reshape(147, 64).to(dev).contiguous(), 'f16': lambda: hip.pack_stem_weights(k.reshape(147, 64).numpy(), dev),
              'f16x3': lambda: hip.pack_stem_weights_x3(k.reshape(147, 64).numpy(), dev)}[family]()
    B = len(imgs)
    for dt, tdt in variants:
        slots = (counter(), counter())
        conv, pool, fused = run_family(family, dt, tdt, weight, bias, canvas, B, 4 * hp, heights, slots)
        want_counts = [0, 0]
        for b, im in enumerate(imgs):
            one = (counter(), counter())
            c1, p1, f1 = run_family(family, dt, tdt, weight, bias, im[None].to(dev).contiguous(), 1, im.shape[0], None, one)
            ho = c1.shape[1]
            assert not torch.isnan(p1.float()).any()
            assert raw(conv[b, :ho]) == raw(c1[0]), (family, dt, b, 'conv rows')
            assert bool(torch.isnan(conv[b, ho:].float()).all()), (family, dt, b, 'rows past the image were written')
            assert raw(pool[b]) == raw(p1[0]), (family, dt, b, 'pooled map, two launches')
            if fused is not None:
                assert raw(f1[0]) == raw(p1[0])
                assert raw(fused[b]) == raw(p1[0]), (family, dt, b, 'pooled map, fused')
            want_counts = [want_counts[i] + int(one[i].item()) for i in range(2)]
        if family == 'f16x3':
            assert want_counts[0] > 0 and want_counts[0] == want_counts[1]
            assert [int(s.item()) for s in slots] == want_counts


@pytest.mark.parametrize('hp,wd', CLASSES)
def test_ragged_f32_stem_against_torch(hp, wd):
    """ independent of the uniform kernels: the ragged float32 stem against torch conv2d per image, with the bar of
    tests/test_stem_gpu.py::test_stem_matches_torch (f16 output: 2^-10 |ref| + 2e-3), and the ragged pool against torch max_pool2d of the map the
    stem stored (max is exact: equality) """
    imgs, canvas, k, bias, heights = stem_case(12, hp, wd)
    dev, B = canvas.device, len(imgs)
    conv, pool, _ = run_family('f32', hip.GPP_F16, torch.float16, k.reshape(147, 64).to(dev).contiguous(), bias, canvas, B, 4 * hp, heights, None)
    for b, im in enumerate(imgs):
        ref = torch.relu(F.conv2d(F.pad(im[None].permute(0, 3, 1, 2), (3, 3, 3, 3)), k.permute(3, 2, 0, 1), bias.cpu(), stride=2)).permute(0, 2, 3, 1)[0]
        ho, wo, hpb, wp = shapes_of(im.shape[0], wd)
        assert hpb == hp
        got = conv[b, :ho].float().cpu()
        err = (got - ref).abs()
        print('f32 stem, image', b, 'max err', err.max().item())
        assert bool((err <= 2.0 ** -10 * ref.abs() + 2e-3).all()), err.max().item()
        pt, pl = max((hp - 1) * 2 + 3 - ho, 0), max((wp - 1) * 2 + 3 - wo, 0)
        xp = F.pad(got.permute(2, 0, 1)[None], (pl // 2, pl - pl // 2, pt // 2, pt - pt // 2), value=float('-inf'))
        assert torch.equal(pool[b].float().cpu(), F.max_pool2d(xp, 3, 2)[0].permute(1, 2, 0))


@pytest.mark.parametrize('hp,wd', CLASSES)
def test_ragged_x3_stem_against_float64(hp, wd):
    """ the ragged x3 stem and its fused pool against float64 conv2d (+ max_pool2d) per image, with the bars of
    tests/test_stem_gpu.py::test_x3_stem_matches_float64: |err| <= 1e-5 |ref| + 2e-6 sqrt(147) rms_c, rms(err) <= 5e-7 rms_c + 1e-8 """
    imgs, canvas, k, bias, heights = stem_case(13, hp, wd, decades=True)
    dev, B = canvas.device, len(imgs)
    packed = hip.pack_stem_weights_x3(k.reshape(147, 64).numpy(), dev)
    conv, pool, fused = run_family('f16x3', hip.GPP_F16X3, torch.float32, packed, bias, canvas, B, 4 * hp, heights, (counter(), counter()))
    for b, im in enumerate(imgs):
        x = F.pad(im[None].double().permute(0, 3, 1, 2), (3, 3, 3, 3))
        ref = torch.relu(F.conv2d(x, k.double().permute(3, 2, 0, 1), bias.cpu().double(), stride=2)).permute(0, 2, 3, 1)[0]
        pre = F.conv2d(x, k.double().permute(3, 2, 0, 1), None, stride=2).permute(0, 2, 3, 1)[0]
        ho, wo, hpb, wp = shapes_of(im.shape[0], wd)
        assert hpb == hp
        got = conv[b, :ho].double().cpu()
        assert torch.isfinite(got).all()
        rms_c = pre.reshape(-1, 64).pow(2).mean(dim=0).sqrt()
        err = (got - ref).abs().reshape(-1, 64)
        tol = 1e-5 * ref.abs().reshape(-1, 64) + 2e-6 * 147 ** 0.5 * rms_c[None, :]
        print('x3 stem, image', b, 'max err / rms', (err / rms_c[None, :]).max().item())
        assert bool((err <= tol).all()), (err / rms_c[None, :]).max().item()
        assert bool((err.pow(2).mean(dim=0).sqrt() <= 5e-7 * rms_c + 1e-8).all())
        # the pooled maps: a max over a window moves by no more than the largest tolerance inside the window
        pt, pl = max((hp - 1) * 2 + 3 - ho, 0), max((wp - 1) * 2 + 3 - wo, 0)
        pad = (pl // 2, pl - pl // 2, pt // 2, pt - pt // 2)
        ref_p = F.max_pool2d(F.pad(ref.permute(2, 0, 1)[None], pad, value=float('-inf')), 3, 2)[0].permute(1, 2, 0)
        tol_p = F.max_pool2d(F.pad(tol.reshape(ho, wo, 64).permute(2, 0, 1)[None], pad, value=0.0), 3, 2)[0].permute(1, 2, 0)
        for name, m in (('two launches', pool), ('fused', fused)):
            assert bool(((m[b].double().cpu() - ref_p).abs() <= tol_p).all()), name


# ---------------------------------------------------------------------------------------------------- preprocessing
@pytest.fixture(scope='module')
def kitti_frames():
    # (black / white noise, as tests/test_pose_gpu.py feeds run_network: synthetic weights detect something in it)
    return [(np.random.default_rng(40 + i).integers(0, 2, size=s + (3,)) * 255).astype(np.uint8) for i, s in enumerate(KITTI_SHAPES)]


def calibration(frames, n_planes='100'):
    planes = synthetic.load_plane_database(n_planes).astype(np.float32)
    P_inv = np.stack([synthetic.synthetic_calibration(I.compute_resize_scale(f.shape))[1] for f in frames]).astype(np.float32)
    return P_inv, np.tile(planes[None], (len(frames), 1, 1))


@pytest.fixture(scope='module')
def pose_model_x3():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('GPP_AUTOTUNE', '0')
        yield models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype='f16x3', pose=True)


def test_ragged_preprocess_is_bit_identical_per_image_and_to_the_host_path(pose_model_x3, kitti_frames):
    """ one frame of each KITTI size in one gpp_preprocess_u8_bgr_ragged launch: the rows of image b are gpp_preprocess_u8_bgr's on that frame
    alone and the host path's (utils.image), byte for byte; the rows below it are zero """
    model = pose_model_x3
    P_inv, planes = calibration(kitti_frames)
    order = [2, 0, 3, 1]
    frames = [kitti_frames[i] for i in order]
    plan, scales = model.stage_frames(frames, P_inv[order], planes)
    assert plan.ragged and tuple(plan.images.shape) == (4, 404, 1333, 3) and plan.heights.cpu().tolist() == [403, 402, 404, 403]
    canvas = plan.images.cpu().numpy()
    for b, f in enumerate(frames):
        one, scale = model.stage_frames(f[None], P_inv[order][b:b + 1], planes[:1])
        want = I.resize_image(I.preprocess_image(f))[0]
        h = want.shape[0]
        assert scales[b] == scale == I.compute_resize_scale(f.shape)
        assert canvas[b, :h].tobytes() == one.images.cpu().numpy()[0].tobytes(), b
        assert canvas[b, :h].tobytes() == want.tobytes(), b
        assert not canvas[b, h:].any()


# ---------------------------------------------------------------------------------------------------- model level
def small_batch(seed):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, size=(h, WD, 3)).astype(np.float32) - BGR_MEAN for h in HEIGHTS]
    planes = synthetic.load_plane_database('100').astype(np.float32)
    _, P_inv = synthetic.synthetic_calibration()
    B = len(images)
    return images, np.tile(P_inv[None].astype(np.float32), (B, 1, 1)), np.tile(planes[None], (B, 1, 1))


@pytest.mark.parametrize('dtype', ['f16x3', 'f32', 'f16'])
def test_predict_on_batch_of_a_list_equals_every_image_alone(dtype, monkeypatch):
    """ resnet50 at the small class through predict_on_batch(list): all 8 outputs of image b are those of predict_on_batch on that image alone,
    byte for byte; the same after capture, with a second call whose heights are permuted; one plan serves the mixed calls """
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    model = models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype=dtype)
    images, P_inv, planes = small_batch(5)
    mixed = model.predict_on_batch([images, P_inv, planes])
    perm = [3, 1, 0, 2]
    plan = model.stage_inputs([[images[i] for i in perm], P_inv[perm], planes[perm]])
    model.capture(plan)
    captured = model.predict_on_batch([[images[i] for i in perm], P_inv[perm], planes[perm]])
    again = model.predict_on_batch([images, P_inv, planes])          # the graph, with the first call's heights back in the table
    assert len(model._plans) == 1 and plan.graph is not None
    assert int((mixed[2] > 0.05).sum()) > 0
    for b in range(len(images)):
        alone = model.predict_on_batch([images[b][None], P_inv[b:b + 1], planes[b:b + 1]])
        for k in range(8):
            assert mixed[k][b].tobytes() == alone[k][0].tobytes(), (dtype, b, k)
            assert again[k][b].tobytes() == alone[k][0].tobytes(), (dtype, b, k, 'replayed graph')
            assert captured[k][perm.index(b)].tobytes() == alone[k][0].tobytes(), (dtype, b, k, 'captured, permuted')
    assert len(model._plans) == 1 + len(images)


def fullsize_check(model, frames):
    P_inv, planes = calibration(frames)
    outs, scales = model.predict_on_frames(frames, P_inv, planes)
    (rows, counts), scales_p = model.predict_poses_on_frames(frames, P_inv, planes)
    assert sum(1 for k in model._plans if isinstance(k[1], tuple)) == 1 and len(model._plans) == 1
    assert scales.shape == (4,) and np.array_equal(scales, scales_p)
    assert int(counts.sum()) > 0
    for b, f in enumerate(frames):
        alone, scale = model.predict_on_frames(f[None], P_inv[b:b + 1], planes[b:b + 1])
        (rows1, counts1), scale_p = model.predict_poses_on_frames(f[None], P_inv[b:b + 1], planes[b:b + 1])
        assert scales[b] == scale == scale_p
        for k in range(8):
            assert outs[k][b].tobytes() == alone[k][0].tobytes(), (b, k)
        assert rows[b].tobytes() == rows1[0].tobytes() and counts[b] == counts1[0], b


def test_fullsize_frames_of_the_four_kitti_sizes_in_one_batch(pose_model_x3, kitti_frames):
    """ f16x3 at full size: one batch of four uint8 frames, one of each KITTI size, through predict_on_frames(list) and
    predict_poses_on_frames(list): outputs, pose rows, counts and scales of image b are those of the same call on that frame alone """
    pose_model_x3._plans.clear()
    fullsize_check(pose_model_x3, kitti_frames)


@pytest.mark.slow
def test_fullsize_frames_of_the_four_kitti_sizes_in_one_batch_f32(kitti_frames, monkeypatch):
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    fullsize_check(models.load_model(W.synthetic_weights('resnet50', 1234), backbone_name='resnet50', dtype='f32', pose=True), kitti_frames)


def test_run_network_batch_4_writes_the_bytes_of_batch_1(tmp_path, monkeypatch, kitti_frames):
    """ bin/run_network.py over a directory with the four frame sizes: --batch-size 4 (one ragged call) writes the same KITTI bytes and the same
    .mat bytes as --batch-size 1 (behind the 128-byte MAT-file header, whose text holds the time of writing) """
    from PIL import Image
    from keras_retinanet_3D.bin import run_network
    monkeypatch.setenv('GPP_AUTOTUNE', '0')
    for d in ('img', 'calib', 'b1', 'b4'):
        (tmp_path / d).mkdir()
    P2 = synthetic.KITTI_LIKE_P2
    calib = 'P0: ' + ' '.join(['0'] * 12) + '\nP1: ' + ' '.join(['0'] * 12) + '\nP2: ' + ' '.join('%.12e' % v for v in P2.reshape(-1)) + '\n'
    for k, f in enumerate(kitti_frames):
        Image.fromarray(f[:, :, ::-1]).save(str(tmp_path / 'img' / ('%06d.png' % k)))
        (tmp_path / 'calib' / ('%06d.txt' % k)).write_text(calib)
    common = ['synthetic:1234.h5', str(tmp_path / 'img'), str(tmp_path / 'calib'), synthetic.plane_database_path('1k')]
    run_network.main(common + [str(tmp_path / 'b1'), '--kitti', '--batch-size', '1'])
    run_network.main(common + [str(tmp_path / 'b4'), '--kitti', '--batch-size', '4'])

    def tree(root):
        return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, fs in os.walk(str(root)) for f in fs)
    assert tree(tmp_path / 'b1') == tree(tmp_path / 'b4') and len(tree(tmp_path / 'b4')) == 8
    n_lines = 0
    for rel in tree(tmp_path / 'b4'):
        a, b = (tmp_path / 'b1' / rel).read_bytes(), (tmp_path / 'b4' / rel).read_bytes()
        skip = 128 if rel.endswith('.mat') else 0
        assert a[skip:] == b[skip:], rel
        n_lines += a.count(b'\n') if rel.endswith('.txt') else 0
    assert n_lines > 0
