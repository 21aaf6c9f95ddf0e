#!/usr/bin/env python
"""
Fit a pool of road planes to a dataset's LiDAR scans: per frame one consensus fit of the road plane in rectified camera coordinates, the
valid frames' planes written as the (N, 4) .mat that distil_planes.py, polling_ceiling.py and run_network.py read (utils/road_fit.py,
csrc/road_fit.hip).  The fit runs on the GPU; --host runs its NumPy form, which returns the same planes bit for bit.

    fit_plane_pool.py <velodyne dir> <calib dir> <pool.mat> [--hypotheses 1024] [--threshold 0.10] [--region X Y Z]
                      [--height LO HI] [--max-tilt 15] [--min-inliers 100] [--seed 0] [--host] [--report]
                      [--planes-per-frame 1] [--min-share 0.10]

Prints the number of frames, of valid frames and the medians of the inlier count and of the RMS distance; with --report one line per frame.

--planes-per-frame P > 1: after a frame's plane its inliers are taken out and the frame is fitted again, up to P
planes per frame; a later plane needs --min-share of the frame's kept points as inliers.  The pool holds the planes in frame order and
within a frame in round order; --report prints one line per (frame, round) and the summary also gives the number of planes.  Mind --height:
it gates a hypothesis by its distance from the CAMERA ORIGIN, and a far ramp extended back to the camera lies outside 1.0 .. 2.5 m (a road
rising 1 in 16 from 25 m on has d = 3.2 m: it is found with --height 1.0 4.0).

The chain from scans to a scored database:  fit_plane_pool.py -> distil_planes.py -> polling_ceiling.py.
"""
import argparse
import os
import sys

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

import numpy as np

from ..utils import plane_db, road_fit


def parse_args(args):
    d = road_fit.DEFAULTS
    parser = argparse.ArgumentParser(description='Fit a per-frame road-plane pool from LiDAR scans.')
    parser.add_argument('velodyne_dir', help='Directory of velodyne .bin scans.')
    parser.add_argument('calib_dir', help='Directory of the calibration files of the same names (.txt).')
    parser.add_argument('out', help='.MAT file to write: the valid frames\' planes in file order.')
    parser.add_argument('--hypotheses', type=int, default=d['hypotheses'], metavar='H', help='Three-point hypotheses per frame.')
    parser.add_argument('--threshold', type=float, default=d['threshold'], metavar='M', help='Inlier distance in metres.')
    parser.add_argument('--region', type=float, nargs=3, default=list(d['region']), metavar=('X', 'Y', 'Z'),
                        help='The road region in camera metres: |x| <= X, |y| <= Y, 0 < z <= Z (at most 40 8 80).')
    parser.add_argument('--height', type=float, nargs=2, default=list(d['height']), metavar=('LO', 'HI'), help='Camera height band in metres.')
    parser.add_argument('--max-tilt', type=float, default=d['max_tilt'], metavar='DEG', help='Largest angle between the normal and the camera\'s y axis.')
    parser.add_argument('--min-inliers', type=int, default=d['min_inliers'], metavar='N', help='A frame with fewer inliers gives no plane.')
    parser.add_argument('--seed', type=int, default=d['seed'], help='Seed of the draws.')
    parser.add_argument('--host', action='store_true', help='Run the NumPy form instead of the GPU.')
    parser.add_argument('--report', action='store_true', help='Also one line per frame.')
    parser.add_argument('--planes-per-frame', type=int, default=1, metavar='P',
                        help='Up to P planes per frame: peel a plane\'s inliers and fit again.  --height gates by the distance from the camera origin: '
                             'a far ramp needs a wider band (e.g. 1.0 4.0).')
    parser.add_argument('--min-share', type=float, default=road_fit.MIN_SHARE, metavar='S',
                        help='A second or later plane of a frame needs this share (0 .. 1) of the frame\'s kept points as inliers.')
    return parser.parse_args(args)


def report_rounds(args, result):
    """ the printed lines and the file of a run with several planes per frame """
    rec = result['record']
    if args.report:
        for f, name in enumerate(result['frames']):
            for r in range(rec['valid'].shape[1]):
                print('{}  round {}  kept {:7d}  inliers {:7d}  {}'.format(
                    name, r, int(rec['kept'][f, r]), int(rec['inliers'][f, r]),
                    'rms {:.4f} m  plane {:+.6f} {:+.6f} {:+.6f} {:+.6f}'.format(rec['rms'][f, r], *rec['planes'][f, r]) if rec['valid'][f, r]
                    else 'no plane'), flush=True)
    valid = rec['valid']
    if not valid.any():
        sys.exit('fit_plane_pool: none of the {} frames gave a plane'.format(len(result['frames'])))
    plane_db.write_database(args.out, result['planes'])
    print('{}: {} frames, {} valid, {} planes, median inliers {:.0f}, median rms {:.4f} m'.format(
        args.out, len(result['frames']), int(valid[:, 0].sum()), int(valid.sum()), float(np.median(rec['inliers'][valid])),
        float(np.median(rec['rms'][valid]))), flush=True)
    return result


def main(args=None):
    args = parse_args(sys.argv[1:] if args is None else args)
    for d in (args.velodyne_dir, args.calib_dir):
        if not os.path.isdir(d):
            sys.exit('fit_plane_pool: {} is no directory'.format(d))
    options = dict(hypotheses=args.hypotheses, threshold=args.threshold, region=tuple(args.region), height=tuple(args.height),
                   max_tilt=args.max_tilt, min_inliers=args.min_inliers, seed=args.seed)
    try:
        road_fit.resolve_options(**options)
        rounds, _ = road_fit._check_rounds(args.planes_per_frame, args.min_share)
    except ValueError as e:
        sys.exit('fit_plane_pool: {}'.format(e))
    if not any(f.endswith('.bin') for f in os.listdir(args.velodyne_dir)):
        sys.exit('fit_plane_pool: {} holds no .bin scans'.format(args.velodyne_dir))
    try:
        result = road_fit.fit_pool(args.velodyne_dir, args.calib_dir, device=not args.host, planes_per_frame=rounds, min_share=args.min_share,
                                   **options)
    except (ValueError, OSError) as e:
        sys.exit('fit_plane_pool: {}'.format(e))
    rec = result['record']
    if rounds > 1:
        return report_rounds(args, result)
    if args.report:
        for name, ok, kept, inl, rms, plane in zip(result['frames'], rec['valid'], rec['kept'], rec['inliers'], rec['rms'], rec['planes']):
            print('{}  kept {:7d}  inliers {:7d}  {}'.format(name, int(kept), int(inl),
                  'rms {:.4f} m  plane {:+.6f} {:+.6f} {:+.6f} {:+.6f}'.format(rms, *plane) if ok else 'no plane'), flush=True)
    n_valid = int(rec['valid'].sum())
    if n_valid < 1:
        sys.exit('fit_plane_pool: none of the {} frames gave a plane'.format(len(result['frames'])))
    plane_db.write_database(args.out, result['planes'])
    print('{}: {} frames, {} valid, median inliers {:.0f}, median rms {:.4f} m'.format(
        args.out, len(result['frames']), n_valid, float(np.median(rec['inliers'][rec['valid']])), float(np.median(rec['rms'][rec['valid']]))), flush=True)
    return result


if __name__ == '__main__':
    main()
