#!/usr/bin/env python

"""
Score tracks against KITTI tracking labels (not in the reference): CLEAR-MOT for the class Car -- MOTA, MOTP, identity switches,
fragmentations, mostly tracked / mostly lost -- on the optimal assignment of every frame.  Parity with the KITTI
tracking devkit is UNPINNED.

    evaluate_tracking.py label_02/ tracks/ [--device] [--metric image|bev|3d] [--min-overlap 0.5] [--hota] [--idf1] [--json out.json]

The two arguments are directories -- every `.txt` file of the label directory is a sequence, scored against the file of the same name in
the track directory -- or two single files.  Labels are label_02 lines, tracks the lines bin/track_results.py and bin/run_network.py
--track write.  NumPy by default; --device runs csrc/mot_eval.hip.  --hota adds HOTA (parity with TrackEval is
UNPINNED): the columns HOTA DetA AssA DetRe DetPr AssRe AssPr LocA in the table, the per-threshold integers and ratios in --json; with
--device on csrc/hota_eval.hip.  --idf1 adds the identity scores (parity with TrackEval is UNPINNED): the columns
IDF1 IDR IDP in the table, after HOTA's when both are given, and IDTP IDFN IDFP in --json; with --device on csrc/idf1_eval.hip.
"""

import argparse
import json
import os
import sys

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

from ..utils import mot_eval


def add_scoring_arguments(parser, prefix=''):
    """ the options that bin/track_results.py and bin/run_network.py share with this tool """
    parser.add_argument('--{}metric'.format(prefix), dest='mot_metric', choices=list(mot_eval.METRICS), default='image',
                        help='The overlap a pair is judged by: the image box, the bird\'s-eye-view box or the 3-D box.')
    parser.add_argument('--{}min-overlap'.format(prefix), dest='mot_min_overlap', type=float, default=mot_eval.DEFAULTS['min_overlap'],
                        help='A row and a label can be paired when they overlap by at least this much.')
    parser.add_argument('--hota', action='store_true',
                        help='Also score HOTA: eight more columns in the table, the integers of the 19 thresholds in --json.')
    parser.add_argument('--idf1', action='store_true',
                        help='Also score identity: the columns IDF1 IDR IDP in the table, the integers IDTP IDFN IDFP in --json.')


def parse_args(args):
    parser = argparse.ArgumentParser(description='CLEAR-MOT of tracks against KITTI tracking labels, class Car.')
    parser.add_argument('label_path', help='A directory of label_02 files, one per sequence, or one such file.')
    parser.add_argument('track_path', help='The directory of track files of the same names, or one track file.')
    add_scoring_arguments(parser)
    parser.add_argument('--device', action='store_true', help='Run the assignment and the trajectory pass on the GPU.')
    parser.add_argument('--json', dest='json_path', help='Also write the summaries and the trajectory tables to this file.')
    parsed = parser.parse_args(args)
    try:
        mot_eval.check_params(parsed.mot_metric, parsed.mot_min_overlap)
    except ValueError as e:
        parser.error(str(e))
    if os.path.isdir(parsed.label_path) != os.path.isdir(parsed.track_path):
        parser.error('give two files or two directories')
    return parsed


def main(args=None):
    args = parse_args(sys.argv[1:] if args is None else args)
    result = mot_eval.evaluate_tracking(args.label_path, args.track_path, metric=args.mot_metric, min_overlap=args.mot_min_overlap,
                                        device=args.device, hota=args.hota, idf1=args.idf1)
    print(mot_eval.summary_table(result))
    if args.json_path:
        with open(args.json_path, 'w') as f:
            json.dump(mot_eval.result_as_json(result), f, indent=1)
    return result


if __name__ == '__main__':
    main()
