#!/usr/bin/env python
"""
KITTI's object benchmark for the class Car (not in the reference, which scores its modified labels only: bin/evaluate.py): AP of the
image box, the bird's-eye-view box and the 3-D box at Easy / Moderate / Hard, and AOS -- utils/kitti_eval.py, DESIGN.md section 4.17.

    evaluate_kitti.py <label_dir> <result_dir> [--device]
        scores the result files that bin/run_network.py --kitti wrote against ORIGINAL label_2 files of the same names
    evaluate_kitti.py <label_dir> <result_dir> --cuboid-nms {bev,3d} --cuboid-nms-threshold T [--device]
        the same after a greedy NMS of every file's cuboids (utils/cuboid_nms.py): a threshold can be swept over
        one result directory without running the network again
    evaluate_kitti.py <label_dir> --model <path | synthetic:seed> --images <dir> --calibs <dir> --planes <file.mat> [--batch-size N]
        runs the model on the images of the label files and scores its rows without writing them: poses, overlaps and matching on the GPU

Parity with the devkit's evaluate_object.cpp is unpinned: the rules are a restatement.
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

import numpy as np

from ..utils import cuboid_nms, kitti_eval


def parse_args(args):
    parser = argparse.ArgumentParser(description='KITTI object benchmark (Car): AP of the image, BEV and 3-D boxes, and AOS.')
    parser.add_argument('label_dir', help='Directory of ORIGINAL label_2 files.')
    parser.add_argument('result_dir', nargs='?', default=None, help='Directory of KITTI result files (bin/run_network.py --kitti).')
    parser.add_argument('--device', action='store_true', help='Overlaps and matching on the GPU (csrc/kitti_eval.hip); the default is NumPy.')
    parser.add_argument('--model', help='Run this model (a path, or synthetic:<seed>) instead of reading result files.')
    parser.add_argument('--images', help='Directory of the images (--model).')
    parser.add_argument('--calibs', help='Directory of the calibration files (--model).')
    parser.add_argument('--planes', help='.MAT file of the road planes (--model).')
    parser.add_argument('--backbone', default='resnet50')
    parser.add_argument('--dtype', default='f16x3', choices=['f16x3', 'f32', 'bf16x3', 'f16', 'bf16'])
    parser.add_argument('--batch-size', type=int, default=8, help='Images per call (--model).')
    parser.add_argument('--min-overlap', type=float, nargs=3, default=[0.7, 0.7, 0.7], metavar=('IMAGE', 'BEV', '3D'),
                        help='A match needs an overlap above it (KITTI\'s Car: 0.7 each).')
    parser.add_argument('--json', default=None, help='Where the result is written as JSON (default: <result_dir>/kitti_eval.json; '
                                                     'with --model: ./kitti_eval.json).')
    parser.add_argument('--cuboid-nms', choices=['bev', '3d'], default=None,
                        help='Suppress duplicate cuboids before scoring: in score order a detection is dropped when a kept one overlaps its '
                             'cuboid by more than --cuboid-nms-threshold in the bird\'s-eye view (bev) or in 3-D (3d).  With --device on the '
                             'GPU (csrc/cuboid_nms.hip); with --model a stage of the model\'s plan.')
    parser.add_argument('--cuboid-nms-threshold', type=float, default=None, help='Inside (0, 1).  No default: it depends on the checkpoint.')
    parsed = parser.parse_args(args)
    if (parsed.cuboid_nms is None) != (parsed.cuboid_nms_threshold is None):
        parser.error('--cuboid-nms and --cuboid-nms-threshold go together: both or neither')
    if parsed.cuboid_nms is not None and not 0.0 < parsed.cuboid_nms_threshold < 1.0:
        parser.error('--cuboid-nms-threshold must lie inside (0, 1), got {}'.format(parsed.cuboid_nms_threshold))
    if (parsed.result_dir is None) == (parsed.model is None):
        parser.error('give either a result directory or --model')
    if parsed.model is not None and not (parsed.images and parsed.calibs and parsed.planes):
        parser.error('--model needs --images, --calibs and --planes')
    return parsed


def score_model(args):
    """ the model on the images of the label files, batch by batch; every batch leaves a chunk on the device """
    import scipy.io
    from .. import models
    from ..utils import gpp_utils
    from ..utils.image import compute_resize_scale, read_image_bgr
    from .run_network import group_items
    model = models.load_model(args.model, backbone_name=args.backbone, dtype=args.dtype, pose=True,
                              cuboid_nms=None if args.cuboid_nms is None else (args.cuboid_nms, args.cuboid_nms_threshold))
    plane_params = scipy.io.loadmat(args.planes)['road_planes_database']
    names = sorted(f for f in os.listdir(args.label_dir) if f.endswith('.txt'))
    chunks = []
    step = max(args.batch_size, 1)
    for start in range(0, len(names), step):
        items = []
        for fn in names[start:start + step]:
            raw = read_image_bgr(os.path.join(args.images, fn.replace('.txt', '.png')))
            scale = compute_resize_scale(raw.shape)
            _, P_inv = gpp_utils.load_calibration(os.path.join(args.calibs, fn), scale)
            items.append({'raw_image': raw, 'P_inv': P_inv, 'labels': kitti_eval.read_label_file(os.path.join(args.label_dir, fn))})
        for group, ragged in group_items(model, items):          # (a batch of mixed shapes runs as several calls: the chunks then follow the groups)
            frames = (list if ragged else np.stack)([it['raw_image'] for it in group])
            planes = np.tile(plane_params[None], (len(group), 1, 1))
            chunk, _ = model.score_poses_on_frames(frames, np.stack([it['P_inv'] for it in group]), planes, [it['labels'] for it in group])
            chunks.append(chunk)
    return kitti_eval.evaluate_chunks(chunks, args.min_overlap)


def suppressed_rows(args):
    """ --cuboid-nms: the rows of every result file (a missing file: no detections) after the suppression, in the order of the sorted
    label files -- what utils.kitti_eval.evaluate_kitti takes as `rows` """
    rows_list = []
    for f in sorted(f for f in os.listdir(args.label_dir) if f.endswith('.txt')):
        path = os.path.join(args.result_dir, f)
        if not os.path.isfile(path):
            rows_list.append(np.zeros((0, kitti_eval.POSE_COLS), np.float32))
            continue
        rows = kitti_eval.rows_from_results(kitti_eval.read_result_file(path))
        if args.device and rows.shape[0]:
            rows_list.append(cuboid_nms.suppress_rows_device(rows[None], args.cuboid_nms, args.cuboid_nms_threshold)[0][0])
        else:
            rows_list.append(cuboid_nms.suppress_rows_np(rows, args.cuboid_nms, args.cuboid_nms_threshold)[0])
    return rows_list


def main(args=None):
    args = parse_args(sys.argv[1:] if args is None else args)
    if args.model is not None:
        result = score_model(args)
        out = args.json or 'kitti_eval.json'
    else:
        if args.cuboid_nms is not None:
            result = kitti_eval.evaluate_kitti(args.label_dir, rows=suppressed_rows(args), device=args.device, min_overlap=args.min_overlap)
        else:
            result = kitti_eval.evaluate_kitti(args.label_dir, args.result_dir, device=args.device, min_overlap=args.min_overlap)
        out = args.json or os.path.join(args.result_dir, 'kitti_eval.json')
    print(kitti_eval.summary_table(result))
    with open(out, 'w') as f:
        json.dump(kitti_eval.result_as_json(result), f, indent=1)
    return result


if __name__ == '__main__':
    main()
