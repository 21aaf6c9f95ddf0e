"""
ORACLE SUPPORT (test infrastructure): generate tests/golden/resize_*.npz by executing the reference's own image path
/root/reference/keras_retinanet_3D/utils/image.py `resize_image(preprocess_image(x), min_side, max_side)`, UNMODIFIED, with
  * keras  -> oracle/np_tf_shim.py stand-ins (floatx, image_data_format)
  * cv2    -> a stub whose `resize` records fx / fy and returns oracle/image_np.resize (float64, plain loops) of what it was handed
so that the scale rule (:184-195), the order (mean first, then resize), the float32 mean subtraction (:47-60) and the dtype handed to
cv2 come from the reference's own statements.  Only the interpolation comes from the oracle.

Frames are small seeded uint8 noise and the sides are small (48 / 160 or 24 / 80 in place of 800 / 1333), so that no file passes
160 KB (noise does not compress).
The rule `smallest side * scale = min_side` makes one axis of every integer-sided call land on an integer, so the frame whose two
products both land on .5 (33 x 65 at scale 0.5: 16.5 and 32.5) is asked for with min_side = 16.5.

Each file: frame (uint8), min_side, max_side, fx, fy (what cv2.resize was called with), scale (what resize_image returned),
preprocessed (the reference's float32 mean-subtracted image), resized (float64).

Run here only (needs /root/reference):   python oracle/gen_resize_goldens.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import image_np  # noqa: E402
import np_tf_shim  # noqa: E402

np_tf_shim.install()

CALLS = []


def _resize(img, dsize, fx=None, fy=None):
    assert dsize is None
    CALLS.append((fx, fy, img.dtype))
    return image_np.resize(img, fx, fy)


cv2 = types.ModuleType('cv2')
cv2.resize = _resize
sys.modules['cv2'] = cv2

sys.path.insert(0, '/root/reference')
from keras_retinanet_3D.utils import image as ref_image  # noqa: E402

assert ref_image.__file__.startswith('/root/reference/'), ref_image.__file__

# name: (rows, cols, min_side, max_side, seed)
FRAMES = {
    'landscape_up': (21, 75, 48, 160, 11),            # 48 / 21 * 75 = 171 > 160: the max_side branch, scale 160 / 75, upscale
    'landscape_down': (45, 170, 24, 80, 12),          # 24 / 45 * 170 = 91 > 80: the max_side branch, scale 80 / 170, downscale
    'portrait': (75, 23, 48, 160, 13),                # the smallest side is the width; 48 / 23 * 75 = 157 < 160: the min_side branch
    'square': (37, 37, 48, 160, 14),                  # the min_side branch
    'half_both_axes': (33, 65, 16.5, 160, 15),        # scale 0.5: 16.5 -> 16 and 32.5 -> 32 (half up would give 17 x 33)
    'one_row': (1, 40, 48, 160, 16),                  # the max_side branch, 160 / 40 = 4: four rows out of one
}


def main():
    out_dir = os.path.join(ROOT, 'tests', 'golden')
    for name, (rows, cols, min_side, max_side, seed) in FRAMES.items():
        frame = np.random.default_rng(seed).integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
        del CALLS[:]
        pre = ref_image.preprocess_image(frame)
        resized, scale = ref_image.resize_image(pre, min_side=min_side, max_side=max_side)
        assert len(CALLS) == 1 and CALLS[0][2] == np.float32 and pre.dtype == np.float32 and resized.dtype == np.float64
        fx, fy, _ = CALLS[0]
        np.savez_compressed(os.path.join(out_dir, 'resize_{}.npz'.format(name)),
                            frame=frame, min_side=np.array(min_side), max_side=np.array(max_side), fx=np.array(fx), fy=np.array(fy),
                            scale=np.array(scale), preprocessed=pre, resized=resized)
        print('{:16s} {} x {} -> {} x {}  scale {!r}'.format(name, rows, cols, resized.shape[0], resized.shape[1], scale))


if __name__ == '__main__':
    main()
