#!/usr/bin/env python

"""
Track the cuboids of a directory of KITTI result files (not in the reference): the sorted file list is one sequence, every detection gets
an identity that persists from frame to frame and the tracks are written in KITTI's tracking format,

    frame id Car -1 -1 alpha x1 y1 x2 y2 h w l x y z r_y score

The network does not run again: the result files of bin/run_network.py --kitti are read (utils/kitti_eval.read_result_file), so a
threshold can be swept.  On the GPU by default (csrc/track.hip: one launch for the whole sequence); --host uses the NumPy form
(utils/track.track_rows_np) and, without --smooth, writes the same bytes.  --track-assign optimal replaces the greedy association by the
optimal one-to-one assignment of every frame, on the GPU and with --host alike.  --oxts FILE --calib FILE (the
sequence's oxts/<seq>.txt and calib/<seq>.txt, one oxts line per result file) move the carried cuboids into every frame's camera
coordinates before they are matched (gpp_track_ego_f64): a parked car keeps its id from a driving camera.
--track-filter kalman with --track-noise, --track-process and --track-birth-speed gives every track the covariance of its ground-plane
position and velocity (gpp_track_kf_f64), and --metric maha gates at --threshold standard deviations.
--rts smooths the finished tracks before they are written (gpp_track_smooth_f64): a backward Rauch-Tung-Striebel
pass over the same filter gives every tracked detection its smoothed x, z and alpha, and every frame the detector missed inside a track --
up to --max-gap frames in a row, by default the run's --max-age -- a row of its own.  It needs the three noise arguments and works under
any --metric and either filter; it wants the raw rows, so it does not go with --smooth.

    track_results.py result_dir/ tracks.txt --metric dist --threshold 2.0 [--max-age 2] [--min-hits 1] [--smooth] [--host]
                     [--track-assign greedy|optimal] [--oxts oxts/0000.txt --calib calib/0000.txt]
                     [--track-filter kalman --track-noise R0 R1 T0 T1 --track-process QP QV --track-birth-speed V0 [--metric maha]]
                     [--rts [--max-gap G] --track-noise R0 R1 T0 T1 --track-process QP QV --track-birth-speed V0]
                     [--labels label_02/0000.txt [--score-metric image] [--score-min-overlap 0.5] [--hota] [--idf1]]

--labels scores the tracks just written against the sequence's label_02 file (CLEAR-MOT; on the GPU unless
--host) and prints the table of bin/evaluate_tracking.py: a threshold sweep is one loop of this one command.  --hota adds the HOTA columns
(section 4.30), --idf1 the columns IDF1 IDR IDP (section 4.31).
"""

import argparse
import os
import sys

import numpy as np

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

from . import evaluate_tracking
from ..utils import kitti_eval
from ..utils import mot_eval
from ..utils import oxts
from ..utils import track as track_utils
from ..utils import track_smooth


def parse_args(args):
    parser = argparse.ArgumentParser(description='Track the cuboids of a directory of KITTI result files.')
    parser.add_argument('result_dir', help='Directory of KITTI result files, one per frame; their sorted names are the sequence.')
    parser.add_argument('tracks_path', help='The file to write, in KITTI\'s tracking format.')
    parser.add_argument('--metric', '--track', dest='metric', choices=list(track_utils.KF_METRICS), required=True,
                        help='bev / 3d: a detection continues a track when their cuboids overlap by more than --threshold in the bird\'s-eye '
                             'view / in 3-D; dist: when their centres lie closer than --threshold metres on the ground; maha: within --threshold standard '
                             'deviations of the track\'s predicted position (needs --track-filter kalman).')
    track_utils.add_filter_arguments(parser)
    parser.add_argument('--threshold', type=float, required=True, help='No default: it depends on the checkpoint and the frame rate.')
    parser.add_argument('--max-age', type=int, default=track_utils.DEFAULTS['max_age'], help='Frames a track survives without a detection.')
    parser.add_argument('--min-hits', type=int, default=1, help='Only tracks seen in at least this many frames are written.')
    parser.add_argument('--birth-score', type=float, default=track_utils.DEFAULTS['birth_score'],
                        help='Only detections with at least this score start a track.')
    parser.add_argument('--smooth', action='store_true', help='Write the filtered cuboid of tracked detections instead of the detector\'s.')
    parser.add_argument('--track-assign', choices=list(track_utils.ASSIGNS), default='greedy',
                        help='greedy: candidates best first (section 4.28).  optimal: the one-to-one assignment of the least total cost '
                             'per frame (section 4.32): a track does not lose its detection to a neighbour that has another.')
    parser.add_argument('--oxts', default=None, help='The sequence\'s KITTI oxts file, one line per result file: compensate the ego-motion '
                                                     '(section 4.33).  Needs --calib.')
    parser.add_argument('--calib', default=None, help='With --oxts: the sequence\'s tracking calibration file (R_rect, Tr_velo_cam, Tr_imu_velo).')
    parser.add_argument('--host', action='store_true', help='The NumPy form instead of the GPU.')
    track_smooth.add_arguments(parser)
    parser.add_argument('--labels', help='The sequence\'s label_02 file: score the tracks just written and print the CLEAR-MOT table.')
    evaluate_tracking.add_scoring_arguments(parser, 'score-')
    parsed = parser.parse_args(args)
    if (parsed.oxts is None) != (parsed.calib is None):
        parser.error('--oxts and --calib go together: both or neither')
    try:
        parsed.rts_noise = track_smooth.smoother_arguments(parsed, parsed.smooth, parsed.max_age)
        parsed.option = track_utils.check_option(dict({'metric': parsed.metric, 'threshold': parsed.threshold, 'max_age': parsed.max_age,
                                                       'birth_score': parsed.birth_score, 'smooth': parsed.smooth,
                                                       'assign': parsed.track_assign}, **track_smooth.filter_option(parsed)))
        mot_eval.check_params(parsed.mot_metric, parsed.mot_min_overlap)
    except ValueError as e:
        parser.error(str(e))
    return parsed


def read_sequence(result_dir):
    """ (names, rows (N, D, 36) float32): the sorted result files of a directory as pose rows, D = the most detections of a frame """
    names = sorted(fn for fn in os.listdir(result_dir) if fn.endswith('.txt'))
    results = [kitti_eval.read_result_file(os.path.join(result_dir, fn)) for fn in names]
    cars = [r[r[:, 0] == 0] for r in results]
    D = max([len(r) for r in cars] + [1])
    if D > track_utils.MAX_DETECTIONS:
        raise ValueError('a frame has {} detections, the tracker takes {}'.format(D, track_utils.MAX_DETECTIONS))
    rows = [kitti_eval.rows_from_results(r, D) for r in cars]
    return names, np.stack(rows) if rows else np.zeros((0, D, track_utils.POSE_COLS), np.float32)


def main(args=None):
    args = parse_args(sys.argv[1:] if args is None else args)
    names, frames = read_sequence(args.result_dir)
    run = track_utils.track_rows_np if args.host else track_utils.track_rows_device
    if args.oxts is None:
        rows, ids, hits, state = run(frames, args.option)[:4]
    else:
        rows, ids, hits, state = run(frames, args.option, ego=oxts.records_for(args.oxts, args.calib, len(names)))[:4]
    fills = ''
    if args.rts:
        ego = None if args.oxts is None else oxts.records_for(args.oxts, args.calib, len(names))
        rows, ids, hits, n = track_smooth.smooth_tracks(frames, ids, hits, args.rts_noise, args.max_gap, ego=ego, host=args.host)
        fills = ', smoothed with {} fills'.format(n)
    with open(args.tracks_path, 'w') as f:
        for k in range(len(names)):
            f.write(track_utils.tracking_lines(k, rows[k], ids[k], hits[k], args.min_hits))
    print('{} frames, {} tracks, {} births dropped{} -> {}'.format(len(names), int(state['next_id']), int(state['dropped']), fills, args.tracks_path))
    if args.labels:
        result = mot_eval.evaluate_tracking(args.labels, args.tracks_path, metric=args.mot_metric, min_overlap=args.mot_min_overlap,
                                            device=not args.host, hota=args.hota, idf1=args.idf1)
        print(mot_eval.summary_table(result))
        return result


if __name__ == '__main__':
    main()
