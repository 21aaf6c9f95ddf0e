#!/usr/bin/env python
"""
Distil a road-plane database for a dataset: from a pool of candidate planes and the dataset's labels, the K planes that ground-plane
polling on those labels loses least with, in pick order -- every prefix of the file is the best database of its size that the greedy rule
finds (utils/plane_db.py, csrc/plane_db.hip).  Cost table and selection run on the GPU.

    distil_planes.py <label_2 dir> <calib dir> <pool.mat> <out.mat> --planes K [--classes Car [Van]] [--report] [--objective {poll,location}]

Prints one line per power of ten of the prefix and one for the whole file: the objective and, with --report (or for the whole file), the
share of objects whose best plane has all six votes.  bin/polling_ceiling.py scores the result.

--objective location picks for the location error that polling leaves instead (section 4.23): the lines then carry the objective in
metres per object and the mean and median location error of the plane polling would pick.  The default output is unchanged.
"""
import argparse
import os
import sys

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

from ..utils import kitti_eval, plane_db


def parse_args(args):
    parser = argparse.ArgumentParser(description='Distil a road-plane database: the K planes of a pool that polling on a labelled dataset loses least with.')
    parser.add_argument('label_dir', help='Directory of ORIGINAL label_2 files.')
    parser.add_argument('calib_dir', help='Directory of the calibration files of the same names.')
    parser.add_argument('pool', help='.MAT file of candidate planes (key road_planes_database).')
    parser.add_argument('out', help='.MAT file to write: the chosen planes in pick order.')
    parser.add_argument('--planes', type=int, required=True, metavar='K', help='How many planes to pick (the run ends earlier when no plane helps any more).')
    parser.add_argument('--classes', nargs='+', default=['Car'], choices=sorted(k for k in kitti_eval.TYPE_CODES if k != 'DontCare'),
                        help='The label types whose objects count.')
    parser.add_argument('--objective', choices=list(plane_db.OBJECTIVES), default='poll',
                        help="What the picks minimise: polling's own key (votes, then the residual), or the location error of the plane polling would "
                             "pick among the chosen ones (DESIGN.md section 4.23).")
    parser.add_argument('--report', action='store_true', help='Also the six-vote share of every power-of-ten prefix (a shorter run each).')
    return parser.parse_args(args)


def main(args=None):
    import scipy.io
    args = parse_args(sys.argv[1:] if args is None else args)
    pool = scipy.io.loadmat(args.pool)[plane_db.DATABASE_KEY]
    if pool.ndim != 2 or pool.shape[1] != 4 or pool.shape[0] < 1:
        sys.exit('distil_planes: {} holds no (M, 4) pool of planes (shape {})'.format(args.pool, pool.shape))
    if args.planes < 1 or args.planes > pool.shape[0]:
        sys.exit('distil_planes: --planes {} of a pool of {} planes'.format(args.planes, pool.shape[0]))
    det_types = 0
    for name in args.classes:
        det_types |= 1 << kitti_eval.TYPE_CODES[name]
    result = plane_db.distil(args.label_dir, args.calib_dir, pool, args.planes, det_types=det_types, report=args.report,
                             **({'objective': args.objective} if args.objective != 'poll' else {}))
    if result['count'] < 1:
        sys.exit('distil_planes: no plane of the pool serves any of the {} objects'.format(result['objects']))
    plane_db.write_database(args.out, result['planes'])
    for line in plane_db.prefix_report(result):
        print(line, flush=True)
    print('{}: {} of {} planes, {} objects'.format(args.out, result['count'], pool.shape[0], result['objects']), flush=True)
    return result


if __name__ == '__main__':
    main()
