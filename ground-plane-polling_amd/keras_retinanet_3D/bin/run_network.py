#!/usr/bin/env python
"""
Run the network on a directory of images -- the MI355X counterpart of the reference harness
/root/reference/keras_retinanet_3D/bin/run_network.py (same positional arguments, flags, output
tree and file formats):

    run_network.py model_path image_dir calib_dir plane_params_path output_dir
                   [--kitti] [--save-images] [--backbone resnet50] [--batch-size N] [--device-pose]

    <output_dir>/<model name>/outputs/full/<image>.mat     boxes keypoints labels scores locations
                                                           angles dimensions residuals  (:291-292)
    <output_dir>/<model name>/outputs/kitti/<image>.txt    KITTI result lines           (:295-330)
    <output_dir>/<model name>/images/composite/<image>.png only with --save-images: the 2-D picture over the 3-D picture
                                                           (utils/visualization.py; with --device-pose rendered on the GPU, csrc/draw.hip)

Differences, all on the host side: images are processed in batches (--batch-size, default 1 =
the reference's behaviour), the per-detection Python loop of :137-287 is vectorised
(utils.gpp_utils.recover_pose), and `model_path` may be 'synthetic:<seed>' because no trained
weights ship with the reference.  With --device-pose the selection, the pose recovery and the KITTI fields are computed
on the GPU as the last stage of the plan (csrc/pose.hip) and the files are written from its rows.  The pictures of --save-images follow
this package's own integer drawing rules, not cv2's pixels; --image-score-threshold (default 0.4, the
reference's constant) selects what is drawn.
"""

import argparse
import os
import shutil
import sys
import time

# Allow relative imports when being executed as script.
if __name__ == "__main__" and __package__ is None:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    import keras_retinanet_3D.bin  # noqa: F401
    __package__ = "keras_retinanet_3D.bin"

import numpy as np
import scipy.io

from .. import models
from ..utils import cuboid_nms, gpp_utils, visualization
from ..utils import track as track_utils
from ..utils import track_smooth
from ..utils.image import compute_resize_scale, preprocess_image, read_image_bgr, resize_image


def parse_args(args):
    parser = argparse.ArgumentParser(description='Simple script for running the network on a directory of images.')
    parser.add_argument('model_path', help='Path to inference model (or synthetic:<seed>).', type=str)
    parser.add_argument('image_dir', help='Path to directory of input images.', type=str)
    parser.add_argument('calib_dir', help='Path to directory of calibration files.', type=str)
    parser.add_argument('plane_params_path', help='Path to .MAT file containing road planes.', type=str)
    parser.add_argument('output_dir', help='Path to output directory', type=str)
    parser.add_argument('--kitti', help='Include to save results in KITTI format.', action='store_true')
    parser.add_argument('--save-images', help='Include to save result images.', action='store_true')
    parser.add_argument('--backbone', default='resnet50',
                        help='The backbone of the model to load: resnet50 | resnet101 | resnet152 | densenet121 | densenet169 | densenet201 | '
                             'mobilenet{128,160,192,224}_{0.25,0.5,0.75,1.0}, e.g. mobilenet224_1.0.')
    parser.add_argument('--batch-size', help='Images per predict_on_batch call.', type=int, default=1)
    parser.add_argument('--dtype', default='f16x3', choices=['f16x3', 'f32', 'bf16x3', 'f16', 'bf16'],
                        help='Arithmetic of the conv stack (not in the reference CLI).  Default f16x3: the fastest type whose detections, plane '
                             'indices and 3-D corners stay within 1e-3 of the float32 (reference floatx) path; f32 = floatx itself; '
                             'bf16x3 / f16 / bf16 are faster and leave that tolerance.')
    parser.add_argument('--device-pose', action='store_true',
                        help='Pose recovery and KITTI fields on the GPU (not in the reference CLI): the model is loaded with pose=True and '
                             'the .mat and KITTI files are written from the rows of its pose stage, and the pictures of --save-images are rendered '
                             'on the GPU from those rows and the raw frames.')
    parser.add_argument('--image-score-threshold', type=float, default=0.4,
                        help='Detections with a score above it are drawn by --save-images (not in the reference CLI, which fixes 0.4).')
    parser.add_argument('--range-audit', action='store_true',
                        help='Audit the lower range of --dtype f16x3 (not in the reference CLI): the model is loaded with range_audit=True, a '
                             'call whose run left a whole conv-operand map below 2^-9 is answered by the float32 twin, and at the end the five '
                             'smallest maps are printed and <output_dir>/<model name>/range_audit.json is written (per map, the minimum over all calls).')
    parser.add_argument('--cuboid-nms', choices=['bev', '3d'], default=None,
                        help='Suppress duplicate cuboids (not in the reference CLI): in score order a detection is dropped when a kept one overlaps '
                             'its cuboid by more than --cuboid-nms-threshold in the bird\'s-eye view (bev) or in 3-D (3d).  With --device-pose a '
                             'stage of the plan on the GPU (cuboid_nms=(metric, threshold)), otherwise applied on the host before the results are written.')
    parser.add_argument('--cuboid-nms-threshold', type=float, default=None,
                        help='The overlap above which --cuboid-nms drops a detection, inside (0, 1).  No default: it depends on the checkpoint.')
    parser.add_argument('--track', choices=list(track_utils.KF_METRICS), default=None,
                        help='Track the cuboids across the images (not in the reference CLI; needs --device-pose): the sorted image list is one '
                             'sequence, every detection gets an identity that persists from frame to frame (csrc/track.hip, on the GPU behind '
                             'the plan) and <output_dir>/<model name>/outputs/tracking/tracks.txt is written in KITTI\'s tracking format.  A '
                             'detection continues a track when their cuboids overlap by more than --track-threshold in the bird\'s-eye view '
                             '(bev) or in 3-D (3d), when their centres lie closer than --track-threshold metres on the ground (dist), or within '
                             '--track-threshold standard deviations of the track\'s predicted position (maha: needs --track-filter kalman).')
    track_utils.add_filter_arguments(parser)
    parser.add_argument('--track-threshold', type=float, default=None,
                        help='The threshold of --track.  No default: it depends on the checkpoint and the frame rate.')
    parser.add_argument('--track-max-age', type=int, default=track_utils.DEFAULTS['max_age'],
                        help='Frames a track survives without a detection.')
    parser.add_argument('--track-assign', choices=list(track_utils.ASSIGNS), default='greedy',
                        help='How --track associates: greedy (candidates best first) or optimal, the one-to-one assignment of the least total '
                             'cost per frame (gpp_track_optimal_f64, DESIGN.md section 4.32).')
    parser.add_argument('--track-oxts', default=None,
                        help='With --track: the sequence\'s KITTI oxts file (oxts/<seq>.txt), one line per image of the sorted list.  The '
                             'carried cuboids are moved into every frame\'s camera coordinates before they are matched '
                             '(gpp_track_ego_f64, DESIGN.md section 4.33): a parked car keeps its id from a driving camera.  Needs --track-calib.')
    parser.add_argument('--track-calib', default=None,
                        help='With --track-oxts: the sequence\'s tracking calibration file (calib/<seq>.txt: R_rect, Tr_velo_cam, Tr_imu_velo).')
    parser.add_argument('--track-min-hits', type=int, default=1, help='Only tracks seen in at least this many frames are written to tracks.txt.')
    parser.add_argument('--track-smooth', action='store_true',
                        help='Write the filtered cuboid (position, size, r_y, alpha) of tracked detections instead of the detector\'s.')
    track_smooth.add_arguments(parser, '--track-rts', '--track-max-gap')
    parser.add_argument('--tracking-labels', default=None,
                        help='With --track: the sequence\'s KITTI label_02 file.  tracks.txt is scored against it on the GPU (CLEAR-MOT on the '
                             'optimal assignment of every frame, image overlap >= 0.5, csrc/mot_eval.hip) and the table of '
                             'bin/evaluate_tracking.py is printed.')
    parser.add_argument('--hota', action='store_true',
                        help='With --tracking-labels: also score HOTA (csrc/hota_eval.hip) and print its eight columns in the table.')
    parser.add_argument('--idf1', action='store_true',
                        help='With --tracking-labels: also score identity (csrc/idf1_eval.hip) and print IDF1 IDR IDP in the table.')
    parsed = parser.parse_args(args)
    if parsed.tracking_labels is not None and parsed.track is None:
        parser.error('--tracking-labels scores the tracks of --track: it needs --track')
    if parsed.hota and parsed.tracking_labels is None:
        parser.error('--hota scores the tracks against --tracking-labels: it needs --tracking-labels')
    if parsed.idf1 and parsed.tracking_labels is None:
        parser.error('--idf1 scores the tracks against --tracking-labels: it needs --tracking-labels')
    if (parsed.track is None) != (parsed.track_threshold is None):
        parser.error('--track and --track-threshold go together: both or neither')
    if (parsed.track_oxts is None) != (parsed.track_calib is None):
        parser.error('--track-oxts and --track-calib go together: both or neither')
    if parsed.track_oxts is not None and parsed.track is None:
        parser.error('--track-oxts compensates the tracker of --track: it needs --track')
    if parsed.track is None and (parsed.track_filter != 'fixed' or parsed.track_noise is not None or parsed.track_process is not None
                                 or parsed.track_birth_speed is not None):
        parser.error('--track-filter, --track-noise, --track-process and --track-birth-speed set the tracker of --track: they need --track')
    if parsed.track is not None:
        if not parsed.device_pose:
            parser.error('--track follows the pose stage on the GPU: it needs --device-pose')
        if parsed.save_images:
            parser.error('--track does not draw: the composites carry no identities; run --save-images without it')
        try:
            parsed.rts_noise = track_smooth.smoother_arguments(parsed, parsed.track_smooth, parsed.track_max_age)
            track_utils.check_option(track_option(parsed))
        except ValueError as e:
            parser.error(str(e))
    elif parsed.rts or parsed.max_gap is not None:
        parser.error('--track-rts and --track-max-gap smooth the tracks of --track: they need --track')
    if (parsed.cuboid_nms is None) != (parsed.cuboid_nms_threshold is None):
        parser.error('--cuboid-nms and --cuboid-nms-threshold go together: both or neither')
    if parsed.cuboid_nms is not None and not 0.0 < parsed.cuboid_nms_threshold < 1.0:
        parser.error('--cuboid-nms-threshold must lie inside (0, 1), got {}'.format(parsed.cuboid_nms_threshold))
    if parsed.range_audit and parsed.dtype != 'f16x3':
        parser.error('--range-audit audits the IEEE-half pairs of --dtype f16x3, not {}'.format(parsed.dtype))
    return parsed


def track_option(args):
    """ the model's `track` option of the command line, or None """
    if args.track is None:
        return None
    option = {'metric': args.track, 'threshold': args.track_threshold, 'max_age': args.track_max_age, 'smooth': args.track_smooth}
    if args.track_assign == 'optimal':
        option['assign'] = 'optimal'
    if args.track_oxts is not None:
        option['ego'] = True
    option.update(track_smooth.filter_option(args))
    return option


def smoother_option(args):
    """ --track-rts: (the smoother's noise, the largest gap it fills), or None without it """
    return (args.rts_noise, args.max_gap) if args.track is not None and args.rts else None


def make_output_tree(args):
    name = os.path.basename(args.model_path)[:-3]
    output_dir = os.path.join(args.output_dir, name)
    if os.path.isdir(output_dir):
        shutil.rmtree(output_dir)
    os.makedirs(os.path.join(output_dir, 'outputs', 'full'))
    if args.kitti:
        os.mkdir(os.path.join(output_dir, 'outputs', 'kitti'))
    if args.save_images:
        os.makedirs(os.path.join(output_dir, 'images', 'composite'))
    if args.track is not None:
        os.mkdir(os.path.join(output_dir, 'outputs', 'tracking'))
    return output_dir


def load_item(args, fn, on_device):
    """ everything the reference does per image before the timer starts (:91-105); with a model that
    preprocesses on the GPU (predict_on_frames) only the raw frame and the scale are prepared here """
    image_fp = os.path.join(args.image_dir, fn.replace('.txt', '.png'))
    raw_image = read_image_bgr(image_fp)
    if on_device:
        image, scale = None, compute_resize_scale(raw_image.shape)
    else:
        image, scale = resize_image(preprocess_image(raw_image))
    P, P_inv = gpp_utils.load_calibration(os.path.join(args.calib_dir, fn), scale)
    return {'image_fp': image_fp, 'raw_image': raw_image, 'image': image, 'scale': scale, 'P': P, 'P_inv': P_inv}


def write_results(args, output_dir, item, det):
    stem = os.path.basename(item['image_fp'])[:-3]
    outputs = {'boxes': det['boxes'][:, :4], 'keypoints': det['boxes'][:, 4:], 'labels': det['labels'], 'scores': det['scores'],
               'locations': det['locations'], 'angles': det['angles'], 'dimensions': det['dimensions'], 'residuals': det['residuals']}
    scipy.io.savemat(os.path.join(output_dir, 'outputs', 'full', stem + 'mat'), outputs)
    if args.kitti:
        with open(os.path.join(output_dir, 'outputs', 'kitti', stem + 'txt'), 'w') as f:
            f.writelines(gpp_utils.kitti_lines(det, item['raw_image'].shape))
    if args.save_images:
        save_composite(output_dir, item, visualization.composite(item['raw_image'], det, raw_calibration(item), args.image_score_threshold))


def raw_calibration(item):
    """ the calibration in raw-image pixels (reference run_network.py:115): item['P'] carries the image scale """
    s = 1.0 / item['scale']
    return np.dot(np.array([[s, 0.0, 0.0], [0.0, s, 0.0], [0.0, 0.0, 1.0]]), item['P'])


def save_composite(output_dir, item, picture):
    """ images/composite/<image>.png: the 2-D picture over the 3-D picture (reference :334-338) """
    visualization.write_png(os.path.join(output_dir, 'images', 'composite', os.path.basename(item['image_fp'])), picture)


def write_results_from_rows(args, output_dir, item, rows_b, count, picture=None):
    """ write_results for one image's rows of the device pose stage (model.predict_poses_on_batch); picture: its composite, rendered on the
    device (model.predict_composites_on_frames) """
    stem = os.path.basename(item['image_fp'])[:-3]
    if args.cuboid_nms is not None:
        rows_b = cuboid_nms.live_first(rows_b)      # (a suppressed row is padding between the kept ones; count = the kept ones)
    det = gpp_utils.detections_from_rows(rows_b, count)
    outputs = {'boxes': det['boxes'][:, :4], 'keypoints': det['boxes'][:, 4:], 'labels': det['labels'], 'scores': det['scores'],
               'locations': det['locations'], 'angles': det['angles'], 'dimensions': det['dimensions'], 'residuals': det['residuals']}
    scipy.io.savemat(os.path.join(output_dir, 'outputs', 'full', stem + 'mat'), outputs)
    if args.kitti:
        with open(os.path.join(output_dir, 'outputs', 'kitti', stem + 'txt'), 'w') as f:
            f.write(gpp_utils.kitti_lines_from_rows(rows_b, count))
    if args.save_images:
        if picture is None:
            picture = visualization.composite_from_rows(item['raw_image'], rows_b, count, raw_calibration(item), args.image_score_threshold)
        save_composite(output_dir, item, picture)


def group_items(model, items, in_order=False):
    """ the items of one batch in groups that run as one call each (in_order: only neighbours share a group, so that the groups keep
    the items' order -- what a tracker needs).  A model with a ragged form (RetinaNet3D.supports_ragged: the ResNets)
    takes every frame of one height class (utils/image.height_class: the four KITTI frame sizes are one class) in one call; any other
    model takes frames of one raw shape per call, as the reference's batches must be.  Returns [(items, ragged)]: ragged = the
    group mixes raw shapes and goes to the model as a list. """
    from ..utils.image import height_class
    ragged_ok = getattr(model, 'supports_ragged', False)
    groups, last = {}, None
    for n, it in enumerate(items):
        shape = tuple(it['raw_image'].shape)
        key = height_class(shape) if ragged_ok else shape
        if in_order:
            last = (n, key) if last is None or last[1] != key else last
            key = last
        groups.setdefault(key, []).append(it)
    return [(group, len(set(tuple(it['raw_image'].shape) for it in group)) > 1) for group in groups.values()]


def main(args=None):
    if args is None:
        args = sys.argv[1:]
    args = parse_args(args)

    ego = None
    if args.track_oxts is not None:              # (before the model is loaded and the output tree is made: a wrong line count ends here)
        from ..utils import oxts
        ego = oxts.records_for(args.track_oxts, args.track_calib, len(os.listdir(args.calib_dir)))
    model = models.load_model(args.model_path, backbone_name=args.backbone, dtype=args.dtype, pose=args.device_pose, range_audit=args.range_audit,
                              cuboid_nms=(args.cuboid_nms, args.cuboid_nms_threshold) if args.device_pose and args.cuboid_nms is not None else None,
                              track=track_option(args))
    audit = {}               # --range-audit: per map, the report of the call that left it smallest
    plane_params = scipy.io.loadmat(args.plane_params_path)['road_planes_database']
    output_dir = make_output_tree(args)

    files = os.listdir(args.calib_dir)
    if args.track is not None:
        files = sorted(files)                    # the sorted image list is one sequence
        tracks = open(os.path.join(output_dir, 'outputs', 'tracking', 'tracks.txt'), 'w')
        finished = []                            # --track-rts: per frame (rows, ids, hits)
    j = 0
    for start in range(0, len(files), max(args.batch_size, 1)):
        on_device = hasattr(model, 'predict_on_frames')
        items = [load_item(args, fn, on_device) for fn in files[start:start + max(args.batch_size, 1)]]
        # images of one call share a shape, or (a model with a ragged form) a height class; split otherwise
        for group, ragged in group_items(model, items, in_order=args.track is not None):
            stack = list if ragged else np.stack          # a ragged group goes to the model as a list of differently sized frames
            P_inv = np.stack([it['P_inv'] for it in group])
            planes = np.tile(plane_params[None], (len(group), 1, 1))
            t0 = time.time()
            if args.device_pose:
                frames = stack([it['raw_image'] for it in group])
                pictures = [None] * len(group)
                if args.track is not None:
                    if ego is None:
                        (rows, counts, ids, hits), _ = model.predict_tracks_on_frames(frames, P_inv, planes)
                    else:
                        (rows, counts, ids, hits), _ = model.predict_tracks_on_frames(frames, P_inv, planes, ego=ego[j:j + len(group)])
                    for k in range(len(group)):
                        if args.rts:                     # the smoother wants the finished run: the lines are written behind the last frame
                            finished.append((np.array(rows[k], np.float32), np.array(ids[k], np.int32), np.array(hits[k], np.int32)))
                        else:
                            tracks.write(track_utils.tracking_lines(j + k, rows[k], ids[k], hits[k], args.track_min_hits))
                elif args.save_images:
                    P_raw = np.stack([raw_calibration(it) for it in group])
                    (rows, counts), _, pictures = model.predict_composites_on_frames(frames, P_inv, planes, P_raw, args.image_score_threshold)
                else:
                    (rows, counts), _ = model.predict_poses_on_frames(frames, P_inv, planes)
                dt = time.time() - t0
                keep_smallest(audit, model)
                for k, it in enumerate(group):
                    print("Image {}: frame rate: {:.2f}".format(j, len(group) / dt))
                    j += 1
                    write_results_from_rows(args, output_dir, it, rows[k], counts[k], pictures[k])
                continue
            if on_device:
                outputs = model.predict_on_frames(stack([it['raw_image'] for it in group]), P_inv, planes)[0][:8]
            else:
                outputs = model.predict_on_batch([stack([it['image'] for it in group]), P_inv, planes])[:8]
            dt = time.time() - t0
            keep_smallest(audit, model)
            for k, it in enumerate(group):
                print("Image {}: frame rate: {:.2f}".format(j, len(group) / dt))
                j += 1
                det = gpp_utils.recover_pose(gpp_utils.select_detections(outputs, it['scale'], image_index=k))
                if args.cuboid_nms is not None:
                    det, _ = cuboid_nms.suppress_detections(det, args.cuboid_nms, args.cuboid_nms_threshold)
                write_results(args, output_dir, it, det)

    if args.track is not None:
        if args.rts and finished:
            write_smoothed_tracks(tracks, finished, smoother_option(args), ego, args.track_min_hits)
        tracks.close()
    if args.tracking_labels is not None:
        from ..utils import mot_eval
        print(mot_eval.summary_table(mot_eval.evaluate_tracking(args.tracking_labels, os.path.join(output_dir, 'outputs', 'tracking', 'tracks.txt'),
                                                                device=True, hota=args.hota, idf1=args.idf1)))
    if args.range_audit:
        write_range_audit(output_dir, model, audit)


def write_smoothed_tracks(tracks, finished, option, ego, min_hits):
    """ --track-rts: the finished run's per-frame (rows, ids, hits) through the offline smoother on the device,
    then the lines of tracks.txt, the fills among them """
    noise, max_gap = option
    D = max(len(r) for r, _, _ in finished)
    rows = np.full((len(finished), D, track_utils.POSE_COLS), -1.0, np.float32)
    ids, hits = np.full((len(finished), D), -1, np.int32), np.zeros((len(finished), D), np.int32)
    for f, (r, i, h) in enumerate(finished):
        rows[f, :len(r)], ids[f, :len(r)], hits[f, :len(r)] = r, i, h
    rows, ids, hits, fills = track_smooth.smooth_tracks(rows, ids, hits, noise, max_gap, ego=ego)
    for f in range(len(finished)):
        tracks.write(track_utils.tracking_lines(f, rows[f], ids[f], hits[f], min_hits))
    print('tracks smoothed offline: {} fills'.format(fills))


def keep_smallest(audit, model):
    """ --range-audit: fold the report of the call just made into `audit` (per map, the call that left its maximum smallest) """
    for rec in (model.last_range_audit or []) if getattr(model, 'audit', False) else []:
        old = audit.get(rec['name'])
        if old is None or not rec['absmax'] >= old['absmax']:          # (a NaN maximum replaces a number and stays)
            audit[rec['name']] = rec


def write_range_audit(output_dir, model, audit):
    import json
    from ..models.retinanet import RANGE_AUDIT_THRESHOLD
    maps = sorted(audit.values(), key=lambda r: (r['absmax'] != r['absmax'], r['absmax']))
    print('range audit: {} maps, {} flagged (call, map) pairs, {} calls answered by the float32 twin; the five smallest map maxima:'.format(
        len(maps), model.small_magnitude_events, model.range_fallbacks))
    for r in maps[:5]:
        print('  {:<28} max {:<10.4g} {} bits kept, {} of {} live channels below 2^-9{}'.format(
            r['name'], r['absmax'], r['bits'], r['small_channels'], r['live'], '  FLAGGED' if r['flagged'] else ''))
    with open(os.path.join(output_dir, 'range_audit.json'), 'w') as f:
        json.dump({'threshold': RANGE_AUDIT_THRESHOLD, 'small_magnitude_events': model.small_magnitude_events,
                   'range_fallbacks': model.range_fallbacks, 'maps': maps,
                   'unobserved': model.range_audit_unobserved() if maps else []}, f, indent=1)


if __name__ == '__main__':
    main()
