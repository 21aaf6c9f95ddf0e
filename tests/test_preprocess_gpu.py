""" The two preprocessing kernels (csrc/preprocess.hip, csrc/preprocess_ragged.hip) through the C ABI, against the float64 oracle
oracle/image_np.py and the fixtures tests/golden/resize_*.npz: no model, no plan, no tuning.  Tap tables come from utils.image, as the
model's come.  Every output buffer is NaN before a launch; a result is finite, within 1e-4 grey levels of the oracle (the bar derived in
tests/test_image_oracle_cpu.py; the kernels perform the host path's float32 operations) and byte-equal to the host path
utils.image.resize_image(preprocess_image(...)).  The shapes are the small ones at which the kernels had never run: a second, partial
256-column block, downscales, one source row or column, scale 1, portrait, an output narrower than a block, half-way output sizes. """
import numpy as np
import pytest
import torch

from helpers import load_resize_golden
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.utils import image as I
from oracle import image_np as O

pytestmark = pytest.mark.gpu

BAR = 1e-4
MEAN = I.IMAGENET_MEAN_BGR


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run_uniform(frames, scale):
    """ gpp_preprocess_u8_bgr on (B, H, W, 3) uint8 frames with the taps of utils.image: (B, Ho, Wo, 3) float32 """
    B, H, Wd = frames.shape[:3]
    Ho, Wo = int(np.rint(H * scale)), int(np.rint(Wd * scale))
    y0, y1, wy = I._axis_taps(Ho, H, scale)
    x0, x1, wx = I._axis_taps(Wo, Wd, scale)
    for t, n, m in ((y0, H, Ho), (y1, H, Ho), (x0, Wd, Wo), (x1, Wd, Wo)):          # nothing out of range goes to the device
        assert t.shape == (m,) and t.min() >= 0 and t.max() <= n - 1
    assert wy.dtype == wx.dtype == np.float32 and wy.shape == (Ho,) and wx.shape == (Wo,)
    taps = [dev(y0.astype(np.int32)), dev(y1.astype(np.int32)), dev(wy), dev(x0.astype(np.int32)), dev(x1.astype(np.int32)), dev(wx)]
    frames_d = dev(frames)
    out = torch.full((B, Ho, Wo, 3), float('nan'), dtype=torch.float32, device='cuda')
    hip.check(hip.lib().gpp_preprocess_u8_bgr(hip.ptr(frames_d), hip.ptr(out), *[hip.ptr(t) for t in taps], B, H, Wd, Ho, Wo,
                                              float(MEAN[0]), float(MEAN[1]), float(MEAN[2]), hip.stream_ptr()), 'gpp_preprocess_u8_bgr')
    return out.cpu().numpy()


def hold(got, want64, host, what):
    """ finite, within the bar of the oracle, byte-equal to the host path; returns the worst error """
    assert got.shape == want64.shape == host.shape, (what, got.shape, want64.shape, host.shape)
    assert np.all(np.isfinite(got)), what
    err = float(np.max(np.abs(got.astype(np.float64) - want64)))
    print('{}: worst error against the oracle {:.3g}'.format(what, err))
    assert err <= BAR, (what, err)
    assert got.dtype == host.dtype == np.float32 and got.tobytes() == host.tobytes(), what
    return err


UNIFORM = [(2, 11, 300, 1.07327),       # output 12 x 322: two column blocks, the second partial; two different images (batch stride)
           (1, 9, 700, 0.37),           # downscale, output 3 x 259
           (3, 1, 5, 3.0),              # one source row: y0 == y1 == 0 everywhere
           (1, 5, 1, 4.0),              # one source column
           (2, 7, 257, 1.0),            # scale 1: the output is the float32 `u8 - mean`, byte for byte
           (1, 300, 8, 1.5),            # portrait, output narrower than one block, 450 rows
           (1, 33, 65, 0.5),            # 16.5 and 32.5 round to 16 and 32
           (1, 6, 10, 2.5)]             # a further upscale ratio
OUT_SHAPES = [(12, 322), (3, 259), (3, 15), (20, 4), (7, 257), (450, 12), (16, 32), (15, 25)]


@pytest.mark.parametrize('case,out_shape', list(zip(UNIFORM, OUT_SHAPES)), ids=['B{}_{}x{}_s{}'.format(*c) for c in UNIFORM])
def test_uniform_kernel_against_the_oracle(case, out_shape):
    B, H, Wd, scale = case
    frames = noise((B, H, Wd, 3), 1000 + H + Wd)
    got = run_uniform(frames, scale)
    assert got.shape == (B,) + out_shape + (3,)
    want = np.stack([O.resize(O.preprocess(f), scale, scale) for f in frames])
    host = np.stack([I.resize_bilinear(I.preprocess_image(f), scale) for f in frames])
    hold(got, want, host, 'uniform {}'.format(case))
    if B > 1:
        assert not np.array_equal(got[0], got[1])
    if scale == 1.0:
        assert got.tobytes() == I.preprocess_image(frames).tobytes()


@pytest.mark.parametrize('name', ['half_both_axes', 'landscape_down', 'landscape_up', 'one_row', 'portrait', 'square'])
def test_uniform_kernel_against_the_references_fixtures(name):
    g = load_resize_golden(name)
    got = run_uniform(g['frame'][None], I.compute_resize_scale(g['frame'].shape, g['min_side'], g['max_side']))
    host, scale = I.resize_image(I.preprocess_image(g['frame']), g['min_side'], g['max_side'])
    assert scale == g['scale']
    hold(got[0], g['resized'], host, 'fixture {}'.format(name))


# the first five have tap weights that float32 holds exactly (1 / scale = 15/16, 7/8, 7/16, 15/8, 31/32); the sixth (160 / 151) puts rounded
# weights on the ragged path
RAGGED_SHAPES = [(45, 150), (40, 140), (20, 70), (90, 300), (44, 155), (43, 151)]
RAGGED_SIDES = (48, 160)


def run_ragged(frames, filler):
    """ gpp_preprocess_u8_bgr_ragged on frames of one height class; every byte of an input slot past the frame's own h * w * 3 is `filler` """
    shapes = [f.shape[:2] for f in frames]
    (Hp, Wo), heights, scales, taps = I.ragged_taps(shapes, *RAGGED_SIDES)
    B, Hr, Wr, Ho = len(frames), max(s[0] for s in shapes), max(s[1] for s in shapes), 4 * Hp
    y0, y1, wy, x0, x1, wx = taps
    for b, (h, w) in enumerate(shapes):                                          # nothing out of range goes to the device
        assert 1 <= heights[b] <= Ho
        for t, n in ((y0[b], h), (y1[b], h), (x0[b], w), (x1[b], w)):
            assert t.min() >= 0 and t.max() <= n - 1
    assert y0.shape == y1.shape == wy.shape == (B, Ho) and x0.shape == x1.shape == wx.shape == (B, Wo)
    assert all(t.dtype == np.int32 for t in (y0, y1, x0, x1, heights)) and wy.dtype == wx.dtype == np.float32
    raw = np.full((B, Hr * Wr * 3), filler, np.uint8)
    for b, f in enumerate(frames):
        raw[b, :f.size] = f.reshape(-1)
    raw_hw = np.array(shapes, np.int32)
    tensors = [dev(raw_hw), dev(heights)] + [dev(t) for t in taps]
    raw_d = dev(raw)
    out = torch.full((B, Ho, Wo, 3), float('nan'), dtype=torch.float32, device='cuda')
    hip.check(hip.lib().gpp_preprocess_u8_bgr_ragged(hip.ptr(raw_d), hip.ptr(out), *[hip.ptr(t) for t in tensors], B, Hr, Wr, Hp, Ho, Wo,
                                                     float(MEAN[0]), float(MEAN[1]), float(MEAN[2]), hip.stream_ptr()),
              'gpp_preprocess_u8_bgr_ragged')
    return out.cpu().numpy(), (Hp, Wo), heights, scales


def test_ragged_kernel_against_the_oracle_and_reads_nothing_outside_a_frame():
    """ upscales and a downscale of different raw widths on one canvas (class Hp 12, width 160): per image the oracle and the host path; the
    rows below an image exactly zero; the same bytes whatever fills the unused part of every input slot """
    frames = [noise((h, w, 3), 2000 + h) for h, w in RAGGED_SHAPES]
    got, cls, heights, scales = run_ragged(frames, 0)
    assert cls == (12, 160) and heights.tolist() == [48, 46, 46, 48, 45, 46] and got.shape == (6, 48, 160, 3)
    assert [round(s, 3) for s in scales] == [1.067, 1.143, 2.286, 0.533, 1.032, 1.06]
    for b, f in enumerate(frames):
        H = int(heights[b])
        want, scale = O.preprocess_resize(f, *RAGGED_SIDES, loops=True)
        host, host_scale = I.resize_image(I.preprocess_image(f), *RAGGED_SIDES)
        assert scale == host_scale == scales[b]
        hold(got[b, :H], want, host, 'ragged image {} {}'.format(b, f.shape[:2]))
        assert got[b, H:].tobytes() == bytes(got[b, H:].nbytes), b                # +0.0 everywhere below the image
    again, _, _, _ = run_ragged(frames, 255)
    assert again.tobytes() == got.tobytes()


def test_uniform_entry_point_refuses_bad_arguments_before_any_launch():
    lib = hip.lib()
    frames, out = dev(noise((1, 2, 2, 3), 1)), torch.full((1, 2, 2, 3), float('nan'), dtype=torch.float32, device='cuda')
    idx, w = dev(np.zeros((2,), np.int32)), dev(np.zeros((2,), np.float32))
    good = [hip.ptr(frames), hip.ptr(out), hip.ptr(idx), hip.ptr(idx), hip.ptr(w), hip.ptr(idx), hip.ptr(idx), hip.ptr(w)]
    m = [float(v) for v in MEAN]
    for k in range(8):                                                            # each pointer in turn
        args = list(good)
        args[k] = None
        assert lib.gpp_preprocess_u8_bgr(*args, 1, 2, 2, 2, 2, *m, hip.stream_ptr()) == -1, k
    assert lib.gpp_preprocess_u8_bgr(*good, 1, 2, 2, 65536, 2, *m, hip.stream_ptr()) == -1
    assert lib.gpp_preprocess_u8_bgr(*good, 65536, 2, 2, 2, 2, *m, hip.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                            # nothing ran
