""" The image path against an independent float64 oracle, without a GPU: oracle/image_np.py (plain loops, no code shared with the product)
against scipy and PIL, then the product's utils/image.py `resize_image(preprocess_image(u8))` against that oracle and against the fixtures
that the reference's own utils/image.py wrote (oracle/gen_resize_goldens.py -> tests/golden/resize_*.npz).

THE BAR between the product (float32) and the oracle (float64): 1e-4 grey levels, absolute.
  * the values are bounded by 255 - 103.939 = 151.1;
  * about eight float32 roundings of 2^-24 relative fall on such values: one subtraction, and per axis one `1 - w`, two products and one
    sum: 8 * 2^-24 * 151.1 = 7.2e-5;
  * the float32 rounding of the two tap weights adds at most 2^-25 each, times a pixel difference of at most 255: 2 * 2^-25 * 255 = 1.5e-5;
  * together at most about 8.8e-5.
Worst value measured over every product-against-oracle case of this module: 3.7e-5 (801 x 1333 at the default sides; the four KITTI sizes 3.3e-5 - 3.6e-5;
the six fixtures 1.9e-5).

Bilinear interpolation is continuous in the source coordinate: where the oracle's floor and the product's fall on different sides of an
integer coordinate the values still agree.  So values are held, never tap indices.

THE BAR between the oracle and PIL (mode F, exact upscale ratios, non-negative pixels): 2 float32 ulps of the value.  PIL accumulates in
double and stores float32 after each of its two passes: half an ulp of each intermediate, carried through non-negative weights that sum
to 1, is at most 2^-24 of the final value = at most one ulp of it, plus half an ulp for the final store: 1.5 ulps.  (With pixels of both
signs an intermediate can be far larger than the final value and no bound in ulps of the value holds: the frames here are raw grey
levels.  The mean is a constant and plays no part in the pixel-centre convention.)

The two coordinate conventions of the oracle ('float64', which the product documents, and 'cv2_float32', recalled from memory of OpenCV
and unverified) differ by 1.51e-2 - 1.54e-2 grey levels on the four KITTI sizes of seeded noise (printed by the last test). """
import numpy as np
import pytest

from helpers import load_resize_golden, resize_golden_names
from keras_retinanet_3D.utils import image as I
from oracle import image_np as O

BAR = 1e-4
KITTI_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
# one height class (Hp 12, width 160) at 48 / 160; the first five have 1 / scale = 15/16, 7/8, 7/16, 15/8, 31/32: tap weights that float32 holds
# exactly; the sixth (160 / 151) has weights that float32 rounds
RAGGED_SMALL = [(45, 150), (40, 140), (20, 70), (90, 300), (44, 155), (43, 151)]
GRID = KITTI_SHAPES + [(1242, 375), (1, 5), (5, 1), (2, 2), (3000, 4000), (800, 800), (801, 1333), (600, 1400), (37, 53), (480, 640)]


def noise(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)


def worst(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got.astype(np.float64) - want)))


# ---------------------------------------------------------------------------------------------------- the oracle itself

def test_the_output_size_rounds_a_half_to_even():
    assert [O.output_size(n, 0.5) for n in (33, 65, 35, 5, 3, 1)] == [16, 32, 18, 2, 2, 0]
    assert O.output_size(375, 1333 / 1242) == 402 and O.output_size(1242, 1333 / 1242) == 1333
    for n in range(1, 200):
        for s in (0.37, 0.5, 1.0, 1.07327, 1.5, 2.5):
            assert O.output_size(n, s) == int(np.rint(n * s))


def test_the_scale_rule():
    assert O.resize_scale(375, 1242) == 1333 / 1242 and O.resize_scale(480, 640) == 800 / 480 and O.resize_scale(1242, 375) == 1333 / 1242
    assert O.resize_scale(800, 1333) == 1.0 and O.resize_scale(37, 37, 48, 160) == 48 / 37


def test_the_means_are_the_float32_values():
    assert O.MEANS_BGR_F32 == tuple(float(np.float32(m)) for m in (103.939, 116.779, 123.68)) and O.MEANS_BGR_F32[0] != 103.939
    u8 = noise(3, 4, 0)
    pre = O.preprocess(u8)
    assert pre.dtype == np.float64 and pre[1, 2, 1] == float(u8[1, 2, 1]) - float(np.float32(116.779))


@pytest.mark.parametrize('convention', O.CONVENTIONS)
def test_the_vectorised_form_is_the_loops(convention):
    for k, (rows, cols, fx, fy) in enumerate([(7, 9, 1.3, 1.3), (1, 5, 3.0, 3.0), (5, 1, 4.0, 4.0), (2, 2, 2.5, 2.5), (12, 31, 0.37, 0.37),
                                              (33, 65, 0.5, 0.5), (6, 10, 1.0, 1.0), (9, 11, 1.7, 0.6)]):
        img = O.preprocess(noise(rows, cols, 20 + k))
        assert np.array_equal(O.resize(img, fx, fy, convention), O.resize_fast(img, fx, fy, convention)), (rows, cols, fx, fy)
    with pytest.raises(ValueError):
        O.resize(img, 1.0, 1.0, 'float16')


@pytest.mark.parametrize('convention', O.CONVENTIONS)
def test_oracle_against_scipy_map_coordinates(convention):
    """ interpolation and border: scipy's order-1 spline with mode='nearest' at the oracle's own coordinates, to 1e-12 """
    from scipy import ndimage
    top = 0.0
    for k, (rows, cols, s) in enumerate([(7, 9, 1.3), (1, 5, 3.0), (5, 1, 4.0), (2, 2, 2.5), (12, 31, 0.37), (33, 65, 0.5), (6, 10, 1.0),
                                         (37, 53, 1.07327), (20, 8, 1.5), (9, 70, 0.73)]):
        img = O.preprocess(noise(rows, cols, 40 + k))
        got = O.resize(img, s, s, convention)
        ys = np.array([O.source_coordinate(d, s, convention) for d in range(got.shape[0])])
        xs = np.array([O.source_coordinate(d, s, convention) for d in range(got.shape[1])])
        coords = np.stack(np.meshgrid(ys, xs, indexing='ij'))
        want = np.stack([ndimage.map_coordinates(img[:, :, c], coords, order=1, mode='nearest') for c in range(3)], axis=-1)
        top = max(top, worst(got, want))
    print('oracle ({}) against scipy.ndimage.map_coordinates: worst {:.3g}'.format(convention, top))
    assert top <= 1e-12


@pytest.mark.parametrize('ratio,shapes', [(2.0, [(7, 9), (16, 21), (1, 6)]), (1.5, [(8, 10), (2, 2), (20, 6)]), (1.25, [(8, 12), (4, 36)]),
                                          (3.0, [(5, 7), (9, 1), (11, 13)])])
def test_oracle_against_pil_bilinear_at_exact_upscale_ratios(ratio, shapes):
    """ the pixel-centre convention: PIL's BILINEAR on a mode-F image, where its in / out scale is exactly 1 / ratio (PIL antialiases a
    downscale, so only upscales), to 2 float32 ulps of the value (module docstring) """
    from PIL import Image
    top = 0.0
    for k, (rows, cols) in enumerate(shapes):
        grey = noise(rows, cols, 60 + k)[:, :, :1].astype(np.float64)
        want = O.resize(grey, ratio, ratio)[:, :, 0]
        out_r, out_c = int(rows * ratio), int(cols * ratio)
        assert want.shape == (out_r, out_c) and out_r == rows * ratio and out_c == cols * ratio
        im = Image.fromarray(grey[:, :, 0].astype(np.float32))
        assert im.mode == 'F'
        got = np.asarray(im.resize((out_c, out_r), Image.BILINEAR)).astype(np.float64)
        ulps = np.abs(got - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        top = max(top, float(ulps.max()))
    print('oracle against PIL x{}: worst {:.3g} float32 ulps of the value'.format(ratio, top))
    assert top <= 2.0


# ---------------------------------------------------------------------------------------------------- the product against the oracle

def product(u8, min_side=800, max_side=1333):
    return I.resize_image(I.preprocess_image(u8), min_side, max_side)


@pytest.mark.parametrize('shape', GRID, ids=lambda s: '{}x{}'.format(*s))
def test_product_against_oracle_over_the_grid(shape):
    u8 = noise(shape[0], shape[1], 100 + shape[0] + shape[1])
    got, scale = product(u8)
    want, want_scale = O.preprocess_resize(u8)
    assert got.dtype == np.float32 and scale == want_scale
    err = worst(got, want)
    print('product against oracle {} -> {}: worst {:.3g}'.format(shape, got.shape[:2], err))
    assert err <= BAR


@pytest.mark.parametrize('shape,min_side,max_side', [((45, 150), 48, 160), ((40, 140), 48, 160), ((20, 70), 48, 160), ((90, 300), 48, 160),
                                                     ((44, 155), 48, 160), ((43, 151), 48, 160), ((375, 1242), 600, 1000), ((33, 65), 16.5, 160), ((37, 53), 100, 100),
                                                     ((64, 48), 96, 96), ((480, 640), 240, 4000)])
def test_product_against_oracle_at_other_sides(shape, min_side, max_side):
    u8 = noise(shape[0], shape[1], 200 + shape[0])
    got, scale = product(u8, min_side, max_side)
    want, want_scale = O.preprocess_resize(u8, min_side, max_side, loops=shape[0] * shape[1] < 20000)
    assert scale == want_scale
    err = worst(got, want)
    print('product against oracle {} at {} / {} -> {}: worst {:.3g}'.format(shape, min_side, max_side, got.shape[:2], err))
    assert err <= BAR


def test_the_six_fixtures_are_there():
    assert set(resize_golden_names()) >= {'half_both_axes', 'landscape_down', 'landscape_up', 'one_row', 'portrait', 'square'}
    assert load_resize_golden('half_both_axes')['resized'].shape == (16, 32, 3)          # 16.5 and 32.5: half to even
    assert load_resize_golden('one_row')['frame'].shape == (1, 40, 3)


@pytest.mark.parametrize('name', ['half_both_axes', 'landscape_down', 'landscape_up', 'one_row', 'portrait', 'square'])
def test_product_against_the_references_own_statements(name):
    """ scale rule, order, float32 mean subtraction and dtype as the reference's utils/image.py stated them when it wrote the fixture """
    g = load_resize_golden(name)
    assert g['fx'] == g['fy'] == g['scale'] and g['preprocessed'].dtype == np.float32 and g['resized'].dtype == np.float64
    pre = I.preprocess_image(g['frame'])
    assert pre.dtype == np.float32 and np.array_equal(pre, g['preprocessed'])
    assert I.compute_resize_scale(g['frame'].shape, g['min_side'], g['max_side']) == g['scale']
    got, scale = I.resize_image(pre, g['min_side'], g['max_side'])
    assert scale == g['scale'] and got.dtype == np.float32
    err = worst(got, g['resized'])
    # the oracle agrees with the reference's statements too: its exact `u8 - mean` is within half a float32 ulp (2^-17 below 256) of theirs
    own, own_scale = O.preprocess_resize(g['frame'], g['min_side'], g['max_side'], loops=True)
    assert own_scale == g['scale'] and worst(own, g["resized"]) <= 2.0 ** -17 + 1e-12          # (+ float64 noise)
    print('product against fixture {} {} -> {}: worst {:.3g}'.format(name, g['frame'].shape[:2], got.shape[:2], err))
    assert err <= BAR


def apply_taps(pre, y0, y1, wy, x0, x1, wx):
    """ a tap table applied in float64 (the weights are the table's float32 values) """
    wx, wy = wx.astype(np.float64)[None, :, None], wy.astype(np.float64)[:, None, None]
    across = pre[:, x0] * (1.0 - wx) + pre[:, x1] * wx
    return across[y0] * (1.0 - wy) + across[y1] * wy


@pytest.mark.parametrize('shapes,sides', [(RAGGED_SMALL, (48, 160)), (KITTI_SHAPES, (800, 1333))])
def test_row_b_of_the_ragged_tap_tables_gives_image_b(shapes, sides):
    (Hp, W), heights, scales, taps = I.ragged_taps(shapes, *sides)
    top = 0.0
    for b, (rows, cols) in enumerate(shapes):
        u8 = noise(rows, cols, 300 + b)
        want, want_scale = O.preprocess_resize(u8, *sides)
        H = int(heights[b])
        assert want.shape == (H, W, 3) and scales[b] == want_scale and 4 * Hp - 3 <= H <= 4 * Hp
        y0, y1, wy, x0, x1, wx = (t[b] for t in taps)
        for t, n in ((y0[:H], rows), (y1[:H], rows), (x0, cols), (x1, cols)):
            assert t.min() >= 0 and t.max() <= n - 1
        top = max(top, worst(apply_taps(O.preprocess(u8), y0[:H], y1[:H], wy[:H], x0, x1, wx), want))
    print('ragged tap tables {} at {} / {}: worst {:.3g}'.format(shapes, sides[0], sides[1], top))
    assert top <= BAR


# ---------------------------------------------------------------------------------------------------- the two coordinate conventions

def test_the_two_coordinate_conventions_stay_within_the_float32_coordinate_spacing():
    """ 'cv2_float32' (from memory of OpenCV, unverified) against 'float64' (the product's) on the four KITTI sizes: the figure is printed
    and recorded in DESIGN.md; held only below 255 * 2^-24 * (output width) * 2 = the float32 coordinate's spacing at the last column times
    the largest pixel step, with a factor 2 """
    top = 0.0
    for k, (rows, cols) in enumerate(KITTI_SHAPES):
        u8 = noise(rows, cols, 400 + k)
        a, _ = O.preprocess_resize(u8, convention='float64')
        b, _ = O.preprocess_resize(u8, convention='cv2_float32')
        d = worst(a, b)
        print('conventions float64 / cv2_float32 on {} x {} -> {} x {}: worst difference {:.3g} grey levels'.format(rows, cols, a.shape[0], a.shape[1], d))
        assert 0.0 < d < 255.0 * 2.0 ** -24 * a.shape[1] * 2
        top = max(top, d)
    print('conventions float64 / cv2_float32: worst over the four KITTI sizes {:.3g} grey levels'.format(top))
