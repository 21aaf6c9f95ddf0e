#!/usr/bin/env python
"""
The accuracy ceiling of ground-plane polling on real labels, without trained weights: KITTI's Car benchmark of the pipeline fed with
PERFECT 2-D keypoints -- label_2 + calib -> keypoint labels -> polling -> pose -> AP, every stage on the GPU (utils/label_prep.py
polling_ceiling).  One table line per plane database: what the database and the polling cost.

    polling_ceiling.py <label_2 dir> <calib dir> <db.mat> [<db.mat> ...] [--image-dir DIR] [--json FILE]

Without --image-dir every frame counts as 376 x 1242 (KITTI's largest: no label box is clipped).
"""
import argparse
import json
import os
import sys

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

from ..utils import kitti_eval, label_prep


def parse_args(args):
    parser = argparse.ArgumentParser(description='KITTI Car AP of ground-plane polling given perfect 2-D keypoints, per plane database.')
    parser.add_argument('label_dir', help='Directory of ORIGINAL label_2 files.')
    parser.add_argument('calib_dir', help='Directory of the calibration files of the same names.')
    parser.add_argument('databases', nargs='+', help='.MAT files of road planes (key road_planes_database).')
    parser.add_argument('--image-dir', default=None, help='Directory of the images: their real sizes clip the boxes.')
    parser.add_argument('--min-overlap', type=float, nargs=3, default=[0.7, 0.7, 0.7], metavar=('IMAGE', 'BEV', '3D'))
    parser.add_argument('--json', default=None, help='Where the results are written as JSON.')
    return parser.parse_args(args)


def image_sizes(image_dir, label_dir):
    """ {stem: (height, width)} of the images that belong to the label files """
    from PIL import Image
    sizes = {}
    for f in sorted(os.listdir(label_dir)):
        stem = os.path.splitext(f)[0]
        for ext in ('.png', '.jpg'):
            path = os.path.join(image_dir, stem + ext)
            if os.path.isfile(path):
                with Image.open(path) as im:
                    sizes[stem] = (im.height, im.width)
                break
    return sizes


def main(args=None):
    args = parse_args(sys.argv[1:] if args is None else args)
    sizes = image_sizes(args.image_dir, args.label_dir) if args.image_dir else None
    out = {}
    for path in args.databases:
        result = label_prep.polling_ceiling(args.label_dir, args.calib_dir, path, min_overlap=args.min_overlap, image_sizes=sizes)
        print(label_prep.ceiling_line(os.path.basename(path), result), flush=True)
        summary = result.pop('summary')
        out[path] = dict(kitti_eval.result_as_json(result), summary=summary)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
