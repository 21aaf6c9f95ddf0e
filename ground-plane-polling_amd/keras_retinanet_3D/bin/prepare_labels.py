#!/usr/bin/env python
"""
KITTI keypoint ("mod") labels from a stock KITTI download: what the reference makes with MATLAB (label_prep/create_mod_labels.m) --
utils/label_prep.py, DESIGN.md section 4.18.  One mod label file per label_2 file, with the calibration file of the same name; the 20
fields per line that bin/evaluate.py and KittiGenerator read.

    prepare_labels.py <label_2 dir> <calib dir> <out dir> [--device]

--device runs csrc/label_prep.hip instead of NumPy: the same bytes.  Parity with MATLAB itself is unpinned.
"""
import argparse
import os
import sys

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

from ..utils import label_prep


def parse_args(args):
    parser = argparse.ArgumentParser(description='Write the keypoint ("mod") label files of a KITTI label_2 directory.')
    parser.add_argument('label_dir', help='Directory of ORIGINAL label_2 files.')
    parser.add_argument('calib_dir', help='Directory of the calibration files of the same names.')
    parser.add_argument('out_dir', help='Where the mod label files are written (created if missing).')
    parser.add_argument('--device', action='store_true', help='Prepare on the GPU (csrc/label_prep.hip); the default is NumPy.')
    return parser.parse_args(args)


def main(args=None):
    args = parse_args(sys.argv[1:] if args is None else args)
    n = label_prep.write_mod_labels(args.label_dir, args.calib_dir, args.out_dir, device=args.device)
    print('{} label files written to {}'.format(n, args.out_dir))


if __name__ == '__main__':
    main()
