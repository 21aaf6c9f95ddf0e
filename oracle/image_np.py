"""
ORACLE (test infrastructure, not product code): float64 restatement of the reference's image path
`resize_image(preprocess_image(x), min_side, max_side)` (reference utils/image.py:36-62 and :174-200), written as plain loops per
output pixel.  It shares no code with the product's utils/image.py: the tests compare the two.

What it states, and where each rule comes from:
  * means      the float32 values of 103.939, 116.779, 123.68.  The reference subtracts Python floats from a float32 array in place
               (:58-60), so its graph sees the float32 means; the oracle gives the exact value of `uint8 - float32 mean`.
  * scale      reference :184-195: min_side / smallest side, unless the largest side would then exceed max_side.
  * order      mean first, then the interpolation of the float image (reference run_network.py: preprocess_image, then resize_image).
  * resize     what the OpenCV documentation gives for cv2.resize(img, None, fx=s, fy=s), INTER_LINEAR:
               dsize = rint(size * s), half to even; source coordinate (d + 0.5) / s - 0.5; the two nearest source pixels, weighted
               by the coordinate's fraction; border replicated: floor < 0 -> index 0 with weight 0, floor >= n - 1 -> index n - 1 with
               weight 0; the horizontal pass first, then the vertical one.

Pinned by (tests/test_image_oracle_cpu.py): scipy.ndimage.map_coordinates(order=1, mode='nearest') on the same coordinates
(interpolation and border), PIL's Image.resize(BILINEAR) on mode-F images at exact upscale ratios (the pixel-centre convention), and
the reference's own statements for scale, order, means and dtype (oracle/gen_resize_goldens.py -> tests/golden/resize_*.npz).
OpenCV itself is absent: "parity unpinned" against a real cv2.resize.

Two conventions of the source coordinate (keyword `convention`):
  'float64'      (d + 0.5) / s - 0.5 in float64: what the product documents and does.
  'cv2_float32'  (float)((d + 0.5) * scale_x - 0.5) with scale_x = 1.0 / s in double, floor and weight taken from that float32 value.
                 THIS FORM IS RECALLED FROM MEMORY of OpenCV's resize.cpp AND HAS NOT BEEN CHECKED AGAINST OPENCV (its source and
                 its binary are both absent).  It is here so that the size of the difference is measured and bounded, not guessed.
"""
import math

import numpy as np

MEANS_BGR_F32 = tuple(float(np.float32(m)) for m in (103.939, 116.779, 123.68))       # the float32 values, held as Python floats
CONVENTIONS = ('float64', 'cv2_float32')


def preprocess(u8):
    """ (h, w, 3) uint8 BGR -> float64: the exact value of `float32(pixel) - float32(mean)` """
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 3 and u8.shape[2] == 3, (u8.dtype, u8.shape)
    out = np.empty(u8.shape, np.float64)
    for c in range(3):
        out[:, :, c] = u8[:, :, c].astype(np.float64) - MEANS_BGR_F32[c]
    return out


def resize_scale(rows, cols, min_side=800, max_side=1333):
    """ the scale rule of the reference's resize_image (utils/image.py:184-195), restated: of the two candidate scales -- the one that
    brings the short side to min_side and the one that brings the long side to max_side -- the first, unless the long side scaled by it
    comes out above max_side """
    short, long_ = (rows, cols) if rows <= cols else (cols, rows)
    to_min, to_max = min_side / short, max_side / long_
    return to_max if long_ * to_min > max_side else to_min


def output_size(size, scale):
    """ dsize of cv2.resize(img, None, fx, fy): the product rounded to the nearest integer, a half to the even one """
    p = size * scale
    f = math.floor(p)
    if p - f > 0.5 or (p - f == 0.5 and f % 2 == 1):
        f += 1
    return int(f)


def source_coordinate(d, scale, convention='float64'):
    """ where the centre of output pixel d lies on the source axis, in source pixels """
    if convention == 'float64':
        return (d + 0.5) / scale - 0.5
    if convention == 'cv2_float32':                     # from memory of OpenCV, unverified (module docstring)
        scale_x = 1.0 / scale
        return float(np.float32((d + 0.5) * scale_x - 0.5))
    raise ValueError('convention is one of {}, got {!r}'.format(CONVENTIONS, convention))


def tap(d, src_size, scale, convention='float64'):
    """ (index of the first pixel, index of the second, weight of the second) for output pixel d """
    s = source_coordinate(d, scale, convention)
    i = math.floor(s)
    w = s - i
    if i < 0:
        return 0, 0, 0.0
    if i >= src_size - 1:
        return src_size - 1, src_size - 1, 0.0
    return i, i + 1, w


def resize(img, fx, fy, convention='float64'):
    """ cv2.resize(img, None, fx=fx, fy=fy) of an (h, w, c) image, in float64, one output pixel at a time """
    img = np.asarray(img, dtype=np.float64)
    rows, cols, ch = img.shape
    out_r, out_c = output_size(rows, fy), output_size(cols, fx)
    xt = [tap(d, cols, fx, convention) for d in range(out_c)]
    yt = [tap(d, rows, fy, convention) for d in range(out_r)]
    across = np.empty((rows, out_c, ch), np.float64)                   # the horizontal pass
    for r in range(rows):
        for d in range(out_c):
            a, b, w = xt[d]
            for c in range(ch):
                across[r, d, c] = img[r, a, c] * (1.0 - w) + img[r, b, c] * w
    out = np.empty((out_r, out_c, ch), np.float64)                     # the vertical pass
    for e in range(out_r):
        a, b, w = yt[e]
        for d in range(out_c):
            for c in range(ch):
                out[e, d, c] = across[a, d, c] * (1.0 - w) + across[b, d, c] * w
    return out


def resize_fast(img, fx, fy, convention='float64'):
    """ `resize` with the pixel loops handed to NumPy (the taps still come from `tap`, one at a time): for the frames that the loops
    would take minutes on.  tests/test_image_oracle_cpu.py holds it equal to `resize` at small sizes. """
    img = np.asarray(img, dtype=np.float64)
    rows, cols, _ = img.shape
    out_r, out_c = output_size(rows, fy), output_size(cols, fx)
    xa, xb, xw = (np.array(t) for t in zip(*[tap(d, cols, fx, convention) for d in range(out_c)]))
    ya, yb, yw = (np.array(t) for t in zip(*[tap(d, rows, fy, convention) for d in range(out_r)]))
    xw, yw = xw.astype(np.float64)[None, :, None], yw.astype(np.float64)[:, None, None]
    across = img[:, xa] * (1.0 - xw) + img[:, xb] * xw
    return across[ya] * (1.0 - yw) + across[yb] * yw


def preprocess_resize(u8, min_side=800, max_side=1333, convention='float64', loops=False):
    """ the reference's resize_image(preprocess_image(u8), min_side, max_side) in float64: (image, scale) """
    scale = resize_scale(u8.shape[0], u8.shape[1], min_side, max_side)
    return (resize if loops else resize_fast)(preprocess(u8), scale, scale, convention), scale
