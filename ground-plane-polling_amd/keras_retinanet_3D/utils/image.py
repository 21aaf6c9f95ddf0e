"""
Host-side image handling of the inference harness (reference utils/image.py:26-62,174-200):
read as BGR, subtract the ImageNet mean, resize so that the short side is 800 unless the long
side would exceed 1333.  The augmentation helpers of the reference file are training-only and
out of scope.

cv2 is not available in this image; `resize_image` restates cv2.resize(img, None, fx=s, fy=s)
(INTER_LINEAR: dsize = round(size * s), source coordinate (d + 0.5) / s - 0.5, border replicated)
in NumPy.  It cannot be checked against OpenCV here.  Those rules are pinned by an independent float64 oracle (oracle/image_np.py, held to
scipy, PIL and the reference's own utils/image.py; tests/test_image_oracle_cpu.py): this module agrees with it to 3.7e-5 grey levels.
The source coordinate is kept in float64.  From memory of OpenCV's resize.cpp -- NOT checked against OpenCV -- cv2 rounds it to float32
before taking floor and weight (the oracle's 'cv2_float32' convention); the two differ by 1.51e-2 - 1.54e-2 grey levels on the four KITTI
sizes of uint8 noise.  That difference is measured and bounded, not pinned.
"""

import numpy as np

IMAGENET_MEAN_BGR = (103.939, 116.779, 123.68)      # utils/image.py:58-60


def read_image_bgr(path):
    """ Read an image in BGR format (utils/image.py:26-33). """
    from PIL import Image
    image = np.asarray(Image.open(path).convert('RGB'))
    return image[:, :, ::-1].copy()


def preprocess_image(x):
    """ float32, ImageNet mean subtracted per BGR channel (utils/image.py:36-62, channels_last). """
    x = x.astype(np.float32)
    x[..., 0] -= 103.939
    x[..., 1] -= 116.779
    x[..., 2] -= 123.68
    return x


def compute_resize_scale(image_shape, min_side=800, max_side=1333):
    """ utils/image.py:184-195 """
    rows, cols = image_shape[0], image_shape[1]
    scale = min_side / min(rows, cols)
    if max(rows, cols) * scale > max_side:
        scale = max_side / max(rows, cols)
    return scale


def _axis_taps(dst_size, src_size, scale):
    """ bilinear taps along one axis: indices i0, i1 and weight of i1 (float32) """
    s = (np.arange(dst_size, dtype=np.float64) + 0.5) / scale - 0.5
    i0 = np.floor(s).astype(np.int64)
    w1 = (s - i0).astype(np.float32)
    lo = i0 < 0
    i0 = np.where(lo, 0, i0)
    w1 = np.where(lo, np.float32(0.0), w1)
    hi = i0 >= src_size - 1
    i1 = np.where(hi, src_size - 1, i0 + 1)
    i0 = np.where(hi, src_size - 1, i0)
    w1 = np.where(hi, np.float32(0.0), w1)
    return i0, i1, w1.astype(np.float32)


def resize_bilinear(img, scale):
    """ cv2.resize(img, None, fx=scale, fy=scale) for float32 HWC input (INTER_LINEAR) """
    rows, cols = img.shape[:2]
    out_r, out_c = int(np.rint(rows * scale)), int(np.rint(cols * scale))
    y0, y1, wy = _axis_taps(out_r, rows, scale)
    x0, x1, wx = _axis_taps(out_c, cols, scale)
    img = np.asarray(img, dtype=np.float32)
    top = img[y0][:, x0] * (1 - wx)[None, :, None] + img[y0][:, x1] * wx[None, :, None]
    bot = img[y1][:, x0] * (1 - wx)[None, :, None] + img[y1][:, x1] * wx[None, :, None]
    return (top * (1 - wy)[:, None, None] + bot * wy[:, None, None]).astype(np.float32)


def resize_image(img, min_side=800, max_side=1333):
    """ (resized image, scale), utils/image.py:174-200 """
    scale = compute_resize_scale(img.shape, min_side, max_side)
    return resize_bilinear(img, scale), scale


# ---------------------------------------------------------------------------------------------------- height classes (ragged batches)
# Images whose resized width is the same and whose resized heights give the same pool1 map run as ONE batch: a height
# class is (Hp, W) = (rows of the pool1 map, resized width); the resized heights 4 Hp - 3 .. 4 Hp belong to it.

def resized_shape(image_shape, min_side=800, max_side=1333):
    """ (resized height, resized width, scale) of a raw image, as resize_image produces them """
    scale = compute_resize_scale(image_shape, min_side, max_side)
    return int(np.rint(image_shape[0] * scale)), int(np.rint(image_shape[1] * scale)), scale


def class_of_resized(height, width):
    """ the height class (Hp, W) of a network input of height x width: Hp = rows of pool1 behind conv1 (7x7 / 2, pad 3) and pool1 (3x3 / 2, 'same') """
    conv_rows = (int(height) - 1) // 2 + 1
    return (conv_rows + 1) // 2, int(width)


def class_height_range(Hp):
    """ (lowest, highest) network-input height of a class; the highest is the row count of the class's canvas """
    return 4 * int(Hp) - 3, 4 * int(Hp)


def height_class(image_shape, min_side=800, max_side=1333):
    """ the height class (Hp, W) of a raw image of image_shape = (rows, cols[, 3]) after resize_image(min_side, max_side) """
    H, W, _ = resized_shape(image_shape, min_side, max_side)
    return class_of_resized(H, W)


def split_by_height_class(image_shapes, min_side=800, max_side=1333):
    """ [(class, [indices into image_shapes])] in the order in which the classes first appear; indices ascending inside a class """
    groups = {}
    for i, shape in enumerate(image_shapes):
        groups.setdefault(height_class(shape, min_side, max_side), []).append(i)
    return list(groups.items())


def ragged_taps(image_shapes, min_side=800, max_side=1333):
    """ the per-image tap tables of gpp_preprocess_u8_bgr_ragged for raw images of ONE height class:
    (cls, heights int32 [B], scales [B], (y0, y1 int32 [B][4 Hp], wy float32 [B][4 Hp], x0, x1 int32 [B][W], wx float32 [B][W])).
    Row b of a table = _axis_taps of image b alone; entries of rows >= heights[b] are zero (never read). """
    classes = split_by_height_class(image_shapes, min_side, max_side)
    if len(classes) != 1:
        raise ValueError('the images span {} height classes ({}): a ragged batch holds one class'.format(
            len(classes), ' and '.join(str(c) for c, _ in classes)))
    (Hp, W), _ = classes[0]
    B, rows = len(image_shapes), 4 * Hp
    y0, y1, x0, x1 = (np.zeros((B, n), np.int32) for n in (rows, rows, W, W))
    wy, wx = np.zeros((B, rows), np.float32), np.zeros((B, W), np.float32)
    heights, scales = np.zeros((B,), np.int32), []
    for b, shape in enumerate(image_shapes):
        H, _, scale = resized_shape(shape, min_side, max_side)
        heights[b] = H
        scales.append(scale)
        y0[b, :H], y1[b, :H], wy[b, :H] = _axis_taps(H, shape[0], scale)
        x0[b], x1[b], wx[b] = _axis_taps(W, shape[1], scale)
    return (Hp, W), heights, scales, (y0, y1, wy, x0, x1, wx)
