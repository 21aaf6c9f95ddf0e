"""
ctypes binding of libgpp_hip.so (C ABI declared in include/gpp.h).

This module takes the place of the reference's operator-alias layer
(/root/reference/keras_retinanet_3D/backend/tensorflow_backend.py:20-156): the layers of this
package call hand-written HIP kernels through it instead of `tensorflow.*`.

There is no CPU fallback.  If the shared library is missing, or no HIP device is present, the
functions below raise; nothing silently routes around the kernels.
"""

import ctypes
import os

_LIB = None
_HERE = os.path.dirname(os.path.abspath(__file__))
# GPP_LIB: alternative build of the library (A/B timing of kernel changes); default = the in-tree build
LIB_PATH = os.environ.get('GPP_LIB') or os.path.normpath(os.path.join(_HERE, '..', '..', 'lib', 'libgpp_hip.so'))
CSRC_DIR = os.path.normpath(os.path.join(_HERE, '..', '..', 'csrc'))

GPP_OK = 0
_ERRORS = {
    -1: 'GPP_ERR_BAD_ARG',
    -2: 'GPP_ERR_WORKSPACE',
    -3: 'GPP_ERR_ALIGN',
    -4: 'GPP_ERR_UNSUPPORTED',
}

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t
c_int64 = ctypes.c_int64
c_double = ctypes.c_double
c_uint32 = ctypes.c_uint32
c_ll = ctypes.c_longlong
_P = ctypes.POINTER


GPP_BF16 = 1
GPP_F16 = 2
GPP_F32 = 3
GPP_BF16X3 = 4
GPP_F16X3 = 5
GPP_MAX_GROUPS = 5
GPP_DRAW_PRIM_WORDS = 16   # int32 words per primitive record of gpp_draw_build (include/gpp.h)
GPP_DRAW_PRIMS_PER_DET = 26
GPP_DRAW_COUNT_WORDS = 4
GPP_POSE_COLS = 36         # float32 values per row of gpp_pose_f32 (include/gpp.h)
GPP_EVAL_MAX_DETECTIONS, GPP_EVAL_MAX_ANNOTATIONS = 1024, 1024      # what gpp_eval_match_f32 takes per image (include/gpp.h)
GPP_EVAL_ANN_COLS, GPP_EVAL_ERR_COLS = 17, 11
GPP_KITTI_MAX_DETECTIONS, GPP_KITTI_MAX_LABELS = 128, 128           # what gpp_kitti_stats_f64 takes per image (include/gpp.h)
GPP_KITTI_MAX_THRESHOLDS, GPP_KITTI_LABEL_COLS = 41, 16
GPP_LABEL_MOD_COLS = 20    # float64 values per row of gpp_label_prep_f64 (include/gpp.h)
GPP_ABSMAX_F32, GPP_ABSMAX_SPLIT_F16, GPP_ABSMAX_SPLIT_BF16 = 1, 2, 3      # gpp_absmax_desc.layout (include/gpp.h)


class GppError(RuntimeError):
    pass


class ConvGroup(ctypes.Structure):
    """ gpp_conv_group (include/gpp.h) """
    _fields_ = [('in_off', c_int64), ('in_bstride', c_int64), ('out_off', c_int64), ('out_bstride', c_int64),
                ('res_off', c_int64), ('res_bstride', c_int64),
                ('H_in', ctypes.c_int32), ('W_in', ctypes.c_int32), ('H_out', ctypes.c_int32), ('W_out', ctypes.c_int32),
                ('H_res', ctypes.c_int32), ('W_res', ctypes.c_int32), ('tile_start', ctypes.c_int32),
                ('row_begin', ctypes.c_int32)]


class ConvDesc(ctypes.Structure):
    """ gpp_conv_desc (include/gpp.h) """
    _fields_ = [('inp', c_void_p), ('weight', c_void_p), ('bias', c_void_p), ('residual', c_void_p),
                ('out', c_void_p), ('zero_page', c_void_p),
                ('dtype', ctypes.c_int32), ('out_f32', ctypes.c_int32),
                ('batch', ctypes.c_int32), ('C_in', ctypes.c_int32), ('C_out', ctypes.c_int32),
                ('KH', ctypes.c_int32), ('KW', ctypes.c_int32), ('stride', ctypes.c_int32),
                ('pad_top', ctypes.c_int32), ('pad_left', ctypes.c_int32),
                ('in_pitch', ctypes.c_int32), ('out_pitch', ctypes.c_int32), ('res_pitch', ctypes.c_int32),
                ('weight_rows', ctypes.c_int32), ('relu', ctypes.c_int32), ('n_groups', ctypes.c_int32),
                ('tile_hint', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('in_bytes', ctypes.c_int32), ('weight_bytes', ctypes.c_int32),
                ('partial', c_void_p), ('partial_bytes', c_int64), ('split_k', ctypes.c_int32), ('partial_rows', ctypes.c_int32),
                ('groups', ConvGroup * GPP_MAX_GROUPS),
                ('x3_split', ctypes.c_int32), ('reserved2', ctypes.c_int32), ('out_scale', c_void_p), ('range_counter', c_void_p),
                ('gather_rows', c_void_p), ('gather_counts', c_void_p), ('guard', c_void_p),
                ('guard_value', ctypes.c_int32), ('reserved3', ctypes.c_int32),
                ('tower_rows', c_void_p), ('tower_counts', c_void_p), ('tower_flag', c_void_p),
                ('tower_tile', ctypes.c_int32), ('reserved4', ctypes.c_int32),
                ('deep_rows', c_void_p), ('deep_counts', c_void_p), ('deep_flag', c_void_p),
                ('deep_tile', ctypes.c_int32), ('lists_after', ctypes.c_int32),
                ('conv_after', ctypes.c_int32), ('conv_before', ctypes.c_int32)]


class PixelListDesc(ctypes.Structure):
    """ gpp_pixel_list_desc (include/gpp.h) """
    _fields_ = [('workspace', c_void_p), ('bitmap', c_void_p), ('rows', c_void_p), ('counts', c_void_p), ('flag', c_void_p),
                ('n_anchors', c_int64)] + \
               [(n, ctypes.c_int32) for n in ('B', 'num_base_anchors', 'lists_per_image', 'n_levels', 'max_rows', 'reserved')] + \
               [('level_pixels', ctypes.c_int32 * GPP_MAX_GROUPS), ('reserved2', ctypes.c_int32)] + \
               [('dilated_bitmap', c_void_p), ('dilated_rows', c_void_p), ('dilated_counts', c_void_p), ('dilated_flag', c_void_p),
                ('level_width', ctypes.c_int32 * GPP_MAX_GROUPS), ('dilated_max_rows', ctypes.c_int32)]


class DeepListDesc(ctypes.Structure):
    """ gpp_deep_list_desc (include/gpp.h) """
    _fields_ = [(n, c_void_p) for n in ('cls_logits', 'marks', 'radius1', 'radius2', 'radius3', 'rows2', 'counts2', 'flag2',
                                        'rows1', 'counts1', 'flag1', 'stats')] + [('n_anchors', c_int64)] + \
               [(n, ctypes.c_int32) for n in ('B', 'num_base_anchors', 'n_levels', 'max_rows', 'tower_max_rows', 'deep_max_rows')] + \
               [('score_thr', c_float), ('reserved', ctypes.c_int32),
                ('level_pixels', ctypes.c_int32 * GPP_MAX_GROUPS), ('level_width', ctypes.c_int32 * GPP_MAX_GROUPS)] + \
               [(n, c_void_p) for n in ('radius4', 'rows0', 'counts0', 'flag0', 'stats0')]


class MobileNetBlockDesc(ctypes.Structure):
    """ gpp_mobilenet_block_desc (include/gpp.h) """
    _fields_ = [('inp', c_void_p), ('dw_weight', c_void_p), ('dw_bias', c_void_p), ('pw_weight', c_void_p), ('pw_bias', c_void_p),
                ('out_scale', c_void_p), ('out', c_void_p)] + \
               [(n, ctypes.c_int32) for n in ('dtype', 'B', 'H', 'W', 'C_in', 'C_out', 'stride', 'in_pitch', 'out_pitch', 'weight_rows',
                                              'tile_hint', 'reserved')]


class MobileNetStemDesc(ctypes.Structure):
    """ gpp_mobilenet_stem_desc (include/gpp.h) """
    _fields_ = [('inp', c_void_p), ('weight', c_void_p), ('bias', c_void_p), ('out', c_void_p)] + \
               [(n, ctypes.c_int32) for n in ('B', 'H', 'W', 'C_out', 'out_pitch', 'reserved')]


class AbsmaxDesc(ctypes.Structure):
    """ gpp_absmax_desc (include/gpp.h) """
    _fields_ = [('inp', c_void_p), ('out', c_void_p), ('M', c_int64), ('pitch', c_int64)] + \
               [(n, ctypes.c_int32) for n in ('C', 'c_off', 'layout', 'reserved')]


GPP_TRACK_MAX_TRACKS, GPP_TRACK_FIELDS = 128, 10   # include/gpp.h, gpp_track_state
GPP_TRACK_EGO_FIELDS = 16                          # gpp_track_ego_f64: one record per frame
GPP_TRACK_MAHA, GPP_TRACK_COV_FIELDS = 3, 10       # gpp_track_kf_f64: the fourth metric, gpp_track_cov's fields


class TrackState(ctypes.Structure):
    """ gpp_track_state (include/gpp.h) """
    _fields_ = [('id1', ctypes.c_int32 * GPP_TRACK_MAX_TRACKS), ('hits', ctypes.c_int32 * GPP_TRACK_MAX_TRACKS),
                ('misses', ctypes.c_int32 * GPP_TRACK_MAX_TRACKS), ('score', c_float * GPP_TRACK_MAX_TRACKS),
                ('box', (ctypes.c_double * GPP_TRACK_MAX_TRACKS) * GPP_TRACK_FIELDS),
                ('next_id', ctypes.c_int32), ('frames', ctypes.c_int32), ('dropped', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class TrackParams(ctypes.Structure):
    """ gpp_track_params (include/gpp.h) """
    _fields_ = [('metric', ctypes.c_int32), ('max_age', ctypes.c_int32), ('smooth', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('threshold', ctypes.c_double), ('gain_a', ctypes.c_double), ('gain_b', ctypes.c_double), ('gain_c', ctypes.c_double),
                ('birth_score', ctypes.c_double)]


class TrackKfParams(ctypes.Structure):
    """ gpp_track_kf_params (include/gpp.h) """
    _fields_ = [(n, ctypes.c_double) for n in ('radial0', 'radial1', 'tangential0', 'tangential1', 'q_pos', 'q_vel', 'birth_speed')] + \
               [('reserved', c_int64)]


GPP_MOT_SCALE_BITS, GPP_MOT_BIG, GPP_MOT_MAX_TRAJECTORIES = 20, 1 << 28, 1024      # include/gpp.h, gpp_mot_assign / gpp_mot_clear
GPP_MOT_FRAME_COUNTS, GPP_MOT_SEQ_COUNTS, GPP_MOT_TRAJ_COLS = 8, 16, 4


class MotParams(ctypes.Structure):
    """ gpp_mot_params (include/gpp.h) """
    _fields_ = [('metric', ctypes.c_int32), ('reserved', ctypes.c_int32), ('min_overlap', ctypes.c_double), ('max_occlusion', ctypes.c_double),
                ('max_truncation', ctypes.c_double), ('min_height', ctypes.c_double)]


# include/gpp.h, gpp_hota_potential / gpp_hota_match / gpp_hota_reduce
GPP_HOTA_LEVELS, GPP_HOTA_HIST, GPP_HOTA_FRAME_COLS, GPP_HOTA_SEQ_COLS, GPP_HOTA_TAB_COLS, GPP_HOTA_SEQ_TAB_COLS = 19, 20, 40, 8, 4, 6
GPP_IDF1_MAX_IDS, GPP_IDF1_SEQ_COLS = 4096, 8                                         # include/gpp.h, gpp_idf1_count / gpp_idf1_assign


class AbsmaxClearDesc(ctypes.Structure):
    """ gpp_absmax_clear_desc (include/gpp.h) """
    _fields_ = [('table', c_void_p), ('n', c_int64)]


# argument lists that several entry points of include/gpp.h share
_SIZE_OUT = _P(c_size_t)                   # where a *_bytes entry point leaves its answer
_HOST_I32 = _P(ctypes.c_int32)             # a host table of int32: seq_start, frame_tab, seq_tab
_CONV = _P(ConvDesc)
_STEM = [c_void_p] * 4 + [c_int] * 4 + [c_void_p]
_STEM_RAGGED = [c_void_p] * 4 + [c_int] * 5 + [c_void_p] * 2
_STEM_X3_RAGGED = [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3
_PACK = [c_void_p, c_void_p, c_size_t]
_WORK = [c_void_p, c_size_t, c_void_p]       # workspace, its bytes, stream
_TILES = [_P(c_int), c_int, _P(c_int)]
_AUTOTUNE = [c_int, c_void_p, _P(c_float)]
_REGISTER, _RELEASE, _RUN = [_P(ctypes.c_int32)], [ctypes.c_int32], [ctypes.c_int32, c_int, c_void_p]
_DETECT_BYTES = [c_int, c_int64, _SIZE_OUT]
_DETECT = [c_void_p] * 4 + [c_int, c_int64, c_int, c_int, c_float, c_float, c_int] + [c_void_p] * 7 + _WORK
_TRACK_HEAD = [c_void_p, c_int, c_int, _HOST_I32, c_int, c_void_p, c_void_p]        # rows, N, D, seq_start, S, state_in, state_out
_TRACK_TAIL = [c_void_p] * 3 + _WORK                                                # out, ids, hits
_TRACK = _TRACK_HEAD + [_P(TrackParams)] + _TRACK_TAIL
_PAIR_BYTES = [c_ll, c_ll, c_int, c_int, _SIZE_OUT]
_FRAME_HEAD = [c_void_p] * 5 + [c_int] * 4 + [_HOST_I32, c_ll, c_ll]                # five maps, N, D, A, metric, frame_tab, cells, vecs
_COST_TABLE = [c_int64, c_int64] + _WORK                                            # pitch, row_offset
_ROAD_FRAMES = [c_void_p] * 4 + [c_uint32, c_void_p] + [c_int] * 4 + [c_double]      # q ... frame_id, seed, winner, F ... H, tq2

# The C ABI of include/gpp.h, in groups: (probe, what a build without it cannot run, {entry point: argument types}).  A group whose probe
# symbol is absent from the loaded library is left unbound: GPP_LIB may name an older build for a same-box A/B (tools/ab_bench.sh), and it
# runs everything but that.  Every entry point returns int, gpp_version its string.  A new entry point is one line in its feature's group
# (a new feature: a new group, probed by its launching function); tests/test_binding_cpu.py holds each line to the header's prototype.
_SIGNATURES = [
    (None, None, {
        'gpp_version': [],
        'gpp_poll_workspace_bytes': [c_int, c_int, c_int, _SIZE_OUT],
        'gpp_poll_f32': [c_void_p] * 5 + [c_int, c_int, c_int, c_int, c_float] + [c_void_p] * 4 + _WORK,
        'gpp_pose_f32': [c_void_p] * 8 + [c_int, c_int, c_float] + [c_void_p] * 3,
        'gpp_conv2d_igemm': [_CONV, c_void_p],
        'gpp_conv2d_flops': [_CONV, _P(c_double)],
        'gpp_conv2d_split_rule': [_CONV, _P(c_int)],
        'gpp_conv2d_workspace_bytes': [_CONV, _SIZE_OUT],
        'gpp_conv2d_tile_candidates': [_CONV] + _TILES,
        'gpp_conv2d_autotune': [_CONV] + _AUTOTUNE,
        'gpp_bottleneck_tail': [_CONV, _CONV, c_int, c_void_p],
        'gpp_bottleneck_block': [_CONV, _CONV, _CONV, c_int, c_void_p],
        'gpp_bottleneck_block_proj': [_CONV, _CONV, _CONV, _CONV, c_int, c_void_p],
        'gpp_stem_conv7x7_bn_relu': _STEM,
        'gpp_stem_conv7x7_bn_relu_mfma': _STEM,
        'gpp_stem_pool_fused_mfma': _STEM,
        'gpp_stem_pack_weights_f16': _PACK,
        'gpp_stem_pack_weights_f16x3': _PACK,
        'gpp_stem_conv7x7_bn_relu_x3': [c_void_p] * 4 + [c_int] * 3 + [c_void_p],
        'gpp_stem_conv7x7_bn_relu_x3_rc': [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 2,
        'gpp_stem_pool_fused_x3': [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 2,
        'gpp_maxpool3x3s2_same': [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p],
        'gpp_relu': [c_void_p, c_void_p, c_int, c_int64, c_void_p],
        'gpp_relu_strided': [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p],
        'gpp_preprocess_u8_bgr': [c_void_p] * 8 + [c_int] * 5 + [c_float] * 3 + [c_void_p],
        # DenseNet: the pre-activation 1x1 conv and the two pools that write into a channel slice
        'gpp_conv2d_preact': [_CONV, c_void_p, c_void_p, c_void_p],
        'gpp_conv2d_preact_tile_candidates': [_CONV] + _TILES,
        'gpp_conv2d_preact_autotune': [_CONV, c_void_p, c_void_p] + _AUTOTUNE,
        'gpp_maxpool3x3s2_pad_f32': [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p],
        'gpp_avgpool2x2_f32': [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p],
        # MobileNet: the fused depthwise-separable block and the 3x3 / 2 stem
        'gpp_mobilenet_block': [_P(MobileNetBlockDesc), c_void_p],
        'gpp_mobilenet_block_tile_candidates': [_P(MobileNetBlockDesc)] + _TILES,
        'gpp_mobilenet_block_autotune': [_P(MobileNetBlockDesc)] + _AUTOTUNE,
        'gpp_mobilenet_stem': [c_void_p] * 4 + [c_int] * 5 + [c_void_p],
        'gpp_mobilenet_depthwise': [c_void_p] * 4 + [c_int] * 7 + [c_void_p],
        # the decode, its one-sort-per-frame form and its stages
        'gpp_detect_workspace_bytes': _DETECT_BYTES,
        'gpp_detect_osf_workspace_bytes': _DETECT_BYTES,
        'gpp_detect_f32': _DETECT,
        'gpp_detect_osf_f32': _DETECT,
        'gpp_detect_stages_f32': [c_int] + _DETECT,
        'gpp_pack_detections': [c_void_p] * 8 + [c_int, c_int, c_void_p, c_void_p],
        'gpp_plan_run': [c_void_p, c_int, c_void_p, c_void_p, c_int],
        'gpp_event_create': [_P(c_void_p)],
        'gpp_event_destroy': [c_void_p],
        'gpp_event_elapsed_ms': [c_void_p, c_void_p, _P(c_float)],
        'gpp_x3_range_events': [_P(ctypes.c_uint64), c_int],
        'gpp_x3_range_snapshot': [c_void_p, c_void_p],
        'gpp_x3_range_snapshot_of': [c_void_p, c_void_p, c_void_p],
    }),
    ('gpp_draw_build', 'the pictures of --save-images (csrc/draw.hip)', {
        'gpp_draw_workspace_bytes': [c_int, c_int, _SIZE_OUT, _SIZE_OUT],
        'gpp_draw_build': [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
        'gpp_draw_raster': [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
    }),
    ('gpp_eval_match_f32', 'evaluate(device=True) (csrc/eval.hip)', {
        'gpp_eval_match_f32': [c_void_p] * 8 + [c_int] * 4 + [c_float, c_int, c_double] + [c_void_p] * 4,
    }),
    ('gpp_cuboid_nms_f64', 'cuboid_nms models (csrc/cuboid_nms.hip)', {
        'gpp_cuboid_nms_f64': [c_void_p, c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p],
    }),
    ('gpp_track_f64', 'track models (csrc/track.hip)', {
        'gpp_track_state_bytes': [_SIZE_OUT],
        'gpp_track_workspace_bytes': [c_int, _SIZE_OUT],
        'gpp_track_f64': _TRACK,
    }),
    ('gpp_track_optimal_f64', "track models with 'assign': 'optimal'", {
        'gpp_track_optimal_f64': _TRACK,
    }),
    ('gpp_track_ego_f64', 'tracking with ego records', {
        'gpp_track_ego_workspace_bytes': [c_int, c_int, _SIZE_OUT],
        'gpp_track_ego_f64': _TRACK_HEAD + [_P(TrackParams), c_void_p, c_int] + _TRACK_TAIL,
    }),
    ('gpp_track_kf_f64', "tracking with 'filter': 'kalman'", {
        'gpp_track_cov_bytes': [_SIZE_OUT],
        'gpp_track_kf_f64': _TRACK_HEAD + [c_void_p, c_void_p, _P(TrackParams), _P(TrackKfParams), c_void_p, c_int] + _TRACK_TAIL,
    }),
    ('gpp_track_smooth_f64', 'the offline smoother of finished tracks (csrc/track_smooth.hip)', {
        'gpp_track_smooth_workspace_bytes': [c_int, c_int, c_ll, _SIZE_OUT],
        'gpp_track_smooth_f64': [c_void_p, c_int, c_int, _P(c_int64), _HOST_I32, _HOST_I32, c_int, _P(TrackKfParams), c_void_p] + [c_void_p] * 4 + _WORK,
    }),
    ('gpp_mot_assign', 'evaluate_tracking(device=True) (csrc/mot_eval.hip)', {
        'gpp_mot_assign': [c_void_p] * 5 + [c_int] * 3 + [_P(MotParams)] + [c_void_p] * 5,
        'gpp_mot_clear_workspace_bytes': [c_int, _SIZE_OUT],
        'gpp_mot_clear': [c_void_p] * 5 + [c_int] * 3 + [_HOST_I32, c_int, c_int] + [c_void_p] * 2 + _WORK,
    }),
    ('gpp_hota_potential', 'the hota=True scores (csrc/hota_eval.hip)', {
        'gpp_hota_workspace_bytes': _PAIR_BYTES,
        'gpp_hota_potential': _FRAME_HEAD + _WORK,
        'gpp_hota_match': _FRAME_HEAD + [c_void_p] * 2 + _WORK,
        'gpp_hota_reduce': [c_void_p, c_int, _HOST_I32, c_int, c_ll, c_ll, c_void_p] + _WORK,
    }),
    ('gpp_idf1_count', 'the idf1=True scores (csrc/idf1_eval.hip)', {
        'gpp_idf1_workspace_bytes': _PAIR_BYTES,
        'gpp_idf1_count': _FRAME_HEAD + _WORK,
        'gpp_idf1_assign': [_HOST_I32, c_int, c_ll, c_ll, c_void_p, c_void_p] + _WORK,
    }),
    ('gpp_kitti_overlaps_f64', 'evaluate_kitti(device=True) and score_poses_on_frames (csrc/kitti_eval.hip)', {
        'gpp_kitti_overlaps_f64': [c_void_p] * 3 + [c_int] * 3 + [c_void_p] * 2,
        'gpp_kitti_stats_f64': [c_void_p] * 4 + [_P(c_double)] + [c_void_p] * 2 + [c_int] * 4 + [c_void_p] * 5,
    }),
    ('gpp_label_prep_f64', 'prepare_device and polling_ceiling (csrc/label_prep.hip)', {
        'gpp_label_prep_f64': [c_void_p] * 4 + [c_int, c_int, ctypes.c_uint, c_int] + [c_void_p] * 7,
    }),
    ('gpp_poll_costs_u16', "utils/plane_db's device entry points (csrc/plane_db.hip)", {
        'gpp_poll_costs_workspace_bytes': [c_int, _SIZE_OUT],
        'gpp_poll_costs_u16': [c_void_p] * 5 + [c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p] + _COST_TABLE,
        'gpp_plane_select_workspace_bytes': [c_int, _SIZE_OUT],
        'gpp_plane_select': [c_void_p, c_int, c_int, c_int64, c_int] + [c_void_p] * 4 + _WORK,
    }),
    ('gpp_pose_costs_u16', "utils/plane_db's objective='location' (DESIGN.md 4.23)", {
        'gpp_pose_costs_u16': [c_void_p] * 6 + [c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p] + _COST_TABLE,
        'gpp_plane_select_polled_workspace_bytes': [c_int, _SIZE_OUT],
        'gpp_plane_select_polled': [c_void_p, c_void_p, c_int, c_int, c_int64, c_int] + [c_void_p] * 5 + _WORK,
    }),
    ('gpp_road_score', "utils/road_fit's device entry points (csrc/road_fit.hip)", {
        'gpp_road_points_i32': [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 3,
        'gpp_road_score': [c_void_p] * 4 + [c_uint32] + [c_int] * 4 + [c_double] * 4 + [c_void_p] * 2,
        'gpp_road_winner': [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
        'gpp_road_moments': _ROAD_FRAMES + [c_void_p, c_void_p],
    }),
    ('gpp_road_peel_i32', 'several road planes per frame (DESIGN.md 4.24)', {
        'gpp_road_peel_workspace_bytes': [c_int, c_int, _SIZE_OUT],
        'gpp_road_peel_i32': _ROAD_FRAMES + [c_void_p] * 2 + _WORK,
    }),
    ('gpp_detect_pixel_lists', 'plans with sparse head outputs (csrc/decode.hip)', {
        'gpp_detect_pixel_lists': [_P(PixelListDesc), c_void_p],
    }),
    ('gpp_detect_deep_lists', 'plans of GPP_SPARSE_TOWER_DEPTH >= 2, which do not build without the deep lists (csrc/decode.hip)', {
        'gpp_detect_deep_lists': [_P(DeepListDesc), c_void_p],
        'gpp_detect_deep_lists_register': [_P(DeepListDesc)] + _REGISTER,
        'gpp_detect_deep_lists_release': _RELEASE,
        'gpp_detect_deep_lists_run': _RUN,
    }),
    ('gpp_conv2d_deferred_register', 'plans of GPP_SPARSE_TOWER_DEPTH >= 4: the layer gpp_conv_desc.conv_after names (csrc/conv_igemm.hip)', {
        'gpp_conv2d_deferred_register': [_CONV] + _REGISTER,
        'gpp_conv2d_deferred_release': _RELEASE,
        'gpp_conv2d_deferred_run': _RUN,
    }),
    ('gpp_channel_absmax', "the range audit of dtype='f16x3': an audit model's plans, whose ops it refuses", {
        'gpp_channel_absmax': [_P(AbsmaxDesc), c_void_p],
        'gpp_absmax_clear': [c_void_p, c_int64, c_void_p],
    }),
    ('gpp_stem_pool_fused_x3_ragged', 'ragged plans (per-image heights read from a device table), whose ops it refuses', {
        'gpp_stem_conv7x7_bn_relu_ragged': _STEM_RAGGED,
        'gpp_stem_conv7x7_bn_relu_mfma_ragged': _STEM_RAGGED,
        'gpp_stem_pool_fused_mfma_ragged': _STEM_RAGGED,
        'gpp_stem_conv7x7_bn_relu_x3_rc_ragged': _STEM_X3_RAGGED,
        'gpp_stem_pool_fused_x3_ragged': _STEM_X3_RAGGED,
        'gpp_maxpool3x3s2_same_ragged': [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, c_void_p],
        'gpp_preprocess_u8_bgr_ragged': [c_void_p] * 10 + [c_int] * 6 + [c_float] * 3 + [c_void_p],
    }),
]


def _declare(lib):
    for probe, _, functions in _SIGNATURES:
        if probe is None or hasattr(lib, probe):
            for name, argtypes in functions.items():
                fn = getattr(lib, name)
                fn.restype = ctypes.c_char_p if name == 'gpp_version' else c_int
                fn.argtypes = argtypes


def build(verbose=False):
    """ Compile libgpp_hip.so in-tree with hipcc for gfx950 (works without a GPU). """
    import subprocess
    cmd = ['make', '-C', CSRC_DIR, '-j4']
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if verbose or out.returncode != 0:
        print(out.stdout)
    if out.returncode != 0:
        raise GppError('building libgpp_hip.so failed (see output above)')


def lib():
    """ The loaded library.  Raises GppError when it has not been built. """
    global _LIB
    if _LIB is None:
        if not os.path.isfile(LIB_PATH):
            raise GppError('{} not found: build it with `make -C {}` (or __graft_entry__.build()); '
                           'there is no CPU fallback for the HIP path'.format(LIB_PATH, CSRC_DIR))
        # PyTorch-ROCm bundles its own libamdhip64.so.7; it must be the HIP runtime already in the
        # process when libgpp_hip.so (linked against the same soname) is loaded, otherwise two
        # runtimes coexist and the kernels see no device (hipErrorNoDevice).
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        _declare(handle)
        _LIB = handle
    return _LIB


def check(rc, what=''):
    if rc == GPP_OK:
        return
    if rc < 0:
        raise GppError('{} failed: {}'.format(what or 'gpp call', _ERRORS.get(rc, rc)))
    raise GppError('{} failed: hipError_t {}'.format(what or 'gpp call', rc))


def require_device():
    """ torch.device('cuda', current) or raise: the product path needs an MI355X. """
    import torch
    if not torch.cuda.is_available():
        raise GppError('no HIP device visible: the ground-plane-polling hot path runs only on the GPU '
                       '(there is no CPU fallback; the CPU oracle under oracle/ is test infrastructure)')
    return torch.device('cuda', torch.cuda.current_device())


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """ Raw device pointer of a contiguous torch tensor (or None). """
    if t is None:
        return None
    assert t.is_contiguous(), 'gpp kernels need dense tensors'
    return ctypes.c_void_p(t.data_ptr())


def _entry(name):
    """ The entry point `name` of the loaded library; GppError when the build lacks it (there is no other path). """
    fn = getattr(lib(), name, None)
    if fn is None:
        what = next(what for _, what, functions in _SIGNATURES if name in functions)
        raise GppError('{} is not in {}: that build runs everything but {}'.format(name, LIB_PATH, what))
    return fn


def _bytes(name, *args):
    """ What the entry point `name`, whose last argument is a size_t*, answers for `args`. """
    n = c_size_t(0)
    check(_entry(name)(*(args + (ctypes.byref(n),))), name)
    return n.value


def _check_tensors(what, dev, want, contiguous=False):
    """ ValueError unless every (tensor, dtype, shape) of `want` is that, on `dev` (and dense, where the entry point `what` needs it) """
    for t, dtype, shape in want:
        if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or (contiguous and not t.is_contiguous()):
            raise ValueError('{}: expected {}{} {} on {}, got {} {} on {}'.format(what, 'contiguous ' if contiguous else '', shape, dtype, dev,
                                                                                 tuple(t.shape), t.dtype, t.device))


def draw_workspace_bytes(B, D):
    """ (bytes of the primitive table, bytes of the raster's workspace) for B images of D rows each """
    prims, work = c_size_t(0), c_size_t(0)
    check(lib().gpp_draw_workspace_bytes(int(B), int(D), ctypes.byref(prims), ctypes.byref(work)), 'gpp_draw_workspace_bytes')
    return prims.value, work.value


def draw_build(rows, P, score_threshold):
    """ gpp_draw_build: rows (B, D, 36) float32 and P (B, 3, 4) float64 on the device -> (prims (B, 26 D, 16) int32, counts (B, 4) int32) """
    import torch
    B, D = int(rows.shape[0]), int(rows.shape[1])
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[2] != GPP_POSE_COLS or P.dtype != torch.float64 or tuple(P.shape) != (B, 3, 4):
        raise ValueError('rows must be (B, D, {}) float32 and P (B, 3, 4) float64, got {} {} and {} {}'.format(
            GPP_POSE_COLS, tuple(rows.shape), rows.dtype, tuple(P.shape), P.dtype))
    prims_bytes, _ = draw_workspace_bytes(B, D)
    prims = torch.empty((B, GPP_DRAW_PRIMS_PER_DET * D, GPP_DRAW_PRIM_WORDS), dtype=torch.int32, device=rows.device)
    assert prims.numel() * 4 == prims_bytes
    counts = torch.zeros((B, GPP_DRAW_COUNT_WORDS), dtype=torch.int32, device=rows.device)
    check(lib().gpp_draw_build(ptr(rows), ptr(P), B, D, float(score_threshold), ptr(prims), ptr(counts), stream_ptr()), 'gpp_draw_build')
    return prims, counts


def draw_raster(frames_u8, raw_hw, Hr, Wr, prims, counts, out_u8, status):
    """ gpp_draw_raster: frames_u8 B slots of Hr Wr 3 bytes, raw_hw (B, 2) int32 -> out_u8 B slots of 2 Hr Wr 3 bytes (only each image's own
    2 h x w x 3 bytes are written), status (B, 4) int32 = the raster's workspace """
    B = int(raw_hw.shape[0])
    if frames_u8.numel() < B * Hr * Wr * 3 or out_u8.numel() < 2 * B * Hr * Wr * 3 or status.numel() < 4 * B or counts.numel() < GPP_DRAW_COUNT_WORDS * B:
        raise ValueError('gpp_draw_raster: a buffer is smaller than B = {} slots of Hr = {}, Wr = {}'.format(B, Hr, Wr))
    check(lib().gpp_draw_raster(ptr(frames_u8), ptr(raw_hw), int(Hr), int(Wr), ptr(prims), ptr(counts), B, ptr(out_u8), ptr(status),
                                stream_ptr()), 'gpp_draw_raster')


def eval_match(boxes, dims, scores, labels, orientations, scales, annotations, ann_counts, num_classes, score_threshold, max_detections,
               iou_threshold):
    """ gpp_eval_match_f32 on the current stream: the decode outputs (B, D, ...) as a plan leaves them, scales (B,) float32, annotations
    (B, A, 17) float64 and ann_counts (B,) int32, all on the device -> (table (B, D, 3) int32, errors (B, D, 11) float64, counts (B,) int32)
    on the device; no synchronisation """
    import torch
    B, D = int(scores.shape[0]), int(scores.shape[1])
    A = int(annotations.shape[1])
    _check_tensors('gpp_eval_match_f32', scores.device, (
        (boxes, torch.float32, (B, D, 12)), (dims, torch.float32, (B, D, 3)), (scores, torch.float32, (B, D)), (labels, torch.int32, (B, D)),
        (orientations, torch.int32, (B, D)), (scales, torch.float32, (B,)), (annotations, torch.float64, (B, A, GPP_EVAL_ANN_COLS)),
        (ann_counts, torch.int32, (B,))))
    table = torch.empty((B, D, 3), dtype=torch.int32, device=scores.device)
    errors = torch.empty((B, D, GPP_EVAL_ERR_COLS), dtype=torch.float64, device=scores.device)
    counts = torch.empty((B,), dtype=torch.int32, device=scores.device)
    check(lib().gpp_eval_match_f32(ptr(boxes), ptr(dims), ptr(scores), ptr(labels), ptr(orientations), ptr(scales), ptr(annotations), ptr(ann_counts),
                                   B, D, A, int(num_classes), float(score_threshold), int(max_detections), float(iou_threshold),
                                   ptr(table), ptr(errors), ptr(counts), stream_ptr()), 'gpp_eval_match_f32')
    return table, errors, counts


def _kitti_check(rows, labels, label_counts, what):
    import torch
    if rows.dim() != 3 or labels.dim() != 3:
        raise ValueError('{}: rows must be (B, D, {}) and labels (B, A, {}), got {} and {}'.format(
            what, GPP_POSE_COLS, GPP_KITTI_LABEL_COLS, tuple(rows.shape), tuple(labels.shape)))
    B, D, A = int(rows.shape[0]), int(rows.shape[1]), int(labels.shape[1])
    _check_tensors(what, rows.device, ((rows, torch.float32, (B, D, GPP_POSE_COLS)), (labels, torch.float64, (B, A, GPP_KITTI_LABEL_COLS)),
                                       (label_counts, torch.int32, (B,))))
    return B, D, A


def kitti_overlaps(rows, labels, label_counts):
    """ gpp_kitti_overlaps_f64 on the current stream: rows (B, D, 36) float32 -- the rows of gpp_pose_f32 --, labels (B, A, 16) float64 and
    label_counts (B,) int32 on the device -> overlaps (B, 4, D, A) float64 on the device (image IoU, BEV IoU, 3-D IoU, image intersection
    over the detection's area); no synchronisation """
    import torch
    B, D, A = _kitti_check(rows, labels, label_counts, 'gpp_kitti_overlaps_f64')
    overlaps = torch.empty((B, 4, D, A), dtype=torch.float64, device=rows.device)
    check(lib().gpp_kitti_overlaps_f64(ptr(rows), ptr(labels), ptr(label_counts), B, D, A, ptr(overlaps), stream_ptr()), 'gpp_kitti_overlaps_f64')
    return overlaps


def kitti_stats(rows, labels, label_counts, overlaps, min_overlap, thresholds=None, n_thresholds=None):
    """ gpp_kitti_stats_f64 on the current stream.  Without thresholds (pass 1): -> (tp_scores (B, 3, 3, A) float32, n_gt (B, 3, 3) int32).
    With thresholds (3, 3, T) float32 and n_thresholds (3, 3) int32 on the device (pass 2): -> (stats (B, 3, 3, T, 3) int32,
    similarity (B, 3, 3, T) float64).  Everything stays on the device; no synchronisation """
    import torch
    B, D, A = _kitti_check(rows, labels, label_counts, 'gpp_kitti_stats_f64')
    dev = rows.device
    _check_tensors('gpp_kitti_stats_f64', dev, ((overlaps, torch.float64, (B, 4, D, A)),))
    mo = (ctypes.c_double * 3)(*[float(v) for v in min_overlap])
    if thresholds is None:
        tp_scores = torch.full((B, 3, 3, A), float('nan'), dtype=torch.float32, device=dev)
        n_gt = torch.zeros((B, 3, 3), dtype=torch.int32, device=dev)
        check(lib().gpp_kitti_stats_f64(ptr(rows), ptr(labels), ptr(label_counts), ptr(overlaps), mo, None, None, B, D, A, 0,
                                        ptr(tp_scores), ptr(n_gt), None, None, stream_ptr()), 'gpp_kitti_stats_f64')
        return tp_scores, n_gt
    T = int(thresholds.shape[2])
    _check_tensors('gpp_kitti_stats_f64', dev, ((thresholds, torch.float32, (3, 3, T)), (n_thresholds, torch.int32, (3, 3))))
    stats = torch.zeros((B, 3, 3, T, 3), dtype=torch.int32, device=dev)
    similarity = torch.zeros((B, 3, 3, T), dtype=torch.float64, device=dev)
    check(lib().gpp_kitti_stats_f64(ptr(rows), ptr(labels), ptr(label_counts), ptr(overlaps), mo, ptr(thresholds), ptr(n_thresholds),
                                    B, D, A, T, None, None, ptr(stats), ptr(similarity), stream_ptr()), 'gpp_kitti_stats_f64')
    return stats, similarity


def cuboid_nms(rows, metric, threshold, out=None, counts=None, suppressor=None):
    """ gpp_cuboid_nms_f64 on the current stream: rows (B, D, 36) float32 on the device -- the rows of gpp_pose_f32 --, metric 0 (bird's-eye
    view) or 1 (3-D) -> (rows_out (B, D, 36) float32, counts (B,) int32, suppressor (B, D) int32) on the device; no synchronisation.
    out: where the rows go (default: a new tensor; `rows` itself: in place) """
    import torch
    if rows.dim() != 3 or rows.dtype != torch.float32 or rows.shape[2] != GPP_POSE_COLS:
        raise ValueError('gpp_cuboid_nms_f64: rows must be (B, D, {}) float32, got {} {}'.format(GPP_POSE_COLS, tuple(rows.shape), rows.dtype))
    B, D = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    out = torch.empty_like(rows) if out is None else out
    counts = torch.zeros((B,), dtype=torch.int32, device=dev) if counts is None else counts
    suppressor = torch.full((B, D), -1, dtype=torch.int32, device=dev) if suppressor is None else suppressor
    _check_tensors('gpp_cuboid_nms_f64', dev, ((out, torch.float32, (B, D, GPP_POSE_COLS)), (counts, torch.int32, (B,)),
                                               (suppressor, torch.int32, (B, D))))
    check(lib().gpp_cuboid_nms_f64(ptr(rows), B, D, int(metric), float(threshold), ptr(out), ptr(counts), ptr(suppressor), stream_ptr()),
          'gpp_cuboid_nms_f64')
    return out, counts, suppressor


def track_state_bytes():
    return _bytes('gpp_track_state_bytes')


def track_workspace_bytes(S):
    return _bytes('gpp_track_workspace_bytes', int(S))


def track_ego_workspace_bytes(S, N):
    return _bytes('gpp_track_ego_workspace_bytes', int(S), int(N))


def track_cov_bytes():
    return _bytes('gpp_track_cov_bytes')


def track(rows, state_in, params, seq_start=None, state_out=None, out=None, ids=None, hits=None, workspace=None, optimal=False, ego=None,
          kf=None, cov_in=None, cov_out=None):
    """ gpp_track_f64 (optimal: gpp_track_optimal_f64, the same arguments) on the current stream: rows (N, D, 36) float32 on the device --
    the rows of gpp_pose_f32 of N frames --, state_in
    (S, gpp_track_state bytes) uint8 on the device, params a TrackParams, seq_start (S + 1) host integers (default: one sequence of all N
    frames) -> (rows_out (N, D, 36) float32, ids (N, D) int32, hits (N, D) int32, state_out) on the device; no synchronisation.
    out: where the rows go (default: a new tensor; `rows` itself: in place); state_out: default a new tensor (`state_in` itself: in place).
    ego: None, or the (N, 16) float64 HOST records of the frames (a NumPy array): gpp_track_ego_f64 with assign = optimal, and a workspace
    of track_ego_workspace_bytes(S, N).
    kf: None, or a TrackKfParams: gpp_track_kf_f64 (with or without `ego`; the workspace is track_ego_workspace_bytes(S, N) either way)
    with cov_in (S, gpp_track_cov bytes) uint8 on the device and cov_out (default: a new tensor; `cov_in` itself: in place)
    -> (rows_out, ids, hits, state_out, cov_out) """
    import torch
    if rows.dim() != 3 or rows.dtype != torch.float32 or rows.shape[2] != GPP_POSE_COLS:
        raise ValueError('gpp_track_f64: rows must be (N, D, {}) float32, got {} {}'.format(GPP_POSE_COLS, tuple(rows.shape), rows.dtype))
    N, D = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    nbytes = track_state_bytes()
    if state_in.dim() != 2 or state_in.dtype != torch.uint8 or state_in.shape[1] != nbytes or state_in.device != dev:
        raise ValueError('gpp_track_f64: the state must be (S, {}) uint8 on {}, got {} {}'.format(nbytes, dev, tuple(state_in.shape), state_in.dtype))
    S = int(state_in.shape[0])
    seq = (ctypes.c_int32 * (S + 1))(*([0, N] if seq_start is None and S == 1 else [int(v) for v in seq_start]))
    covered = S > 0 and seq[0] == 0 and seq[S] == N
    out = (torch.empty_like(rows) if covered else rows.clone()) if out is None else out      # (frames outside every sequence are not written)
    ids = torch.full((N, D), -1, dtype=torch.int32, device=dev) if ids is None else ids
    hits = torch.zeros((N, D), dtype=torch.int32, device=dev) if hits is None else hits
    state_out = torch.empty_like(state_in) if state_out is None else state_out
    if ego is not None:
        import numpy as np
        ego = np.ascontiguousarray(ego, np.float64)
        if ego.shape != (N, GPP_TRACK_EGO_FIELDS):
            raise ValueError('gpp_track_ego_f64: ego must be ({}, {}) float64 on the host, got {}'.format(N, GPP_TRACK_EGO_FIELDS, ego.shape))
    need = track_workspace_bytes(S) if ego is None and kf is None else track_ego_workspace_bytes(S, N)
    if kf is not None:
        cbytes = track_cov_bytes()
        if cov_in is None:
            raise ValueError('gpp_track_kf_f64: the covariance must be ({}, {}) uint8 on {}'.format(S, cbytes, dev))
        cov_out = torch.empty_like(cov_in) if cov_out is None else cov_out
        _check_tensors('gpp_track_kf_f64', dev, ((cov_in, torch.uint8, (S, cbytes)), (cov_out, torch.uint8, (S, cbytes))))
    elif cov_in is not None or cov_out is not None:
        raise ValueError('gpp_track_f64: a covariance belongs to gpp_track_kf_f64 (kf=TrackKfParams)')
    workspace = torch.empty((need,), dtype=torch.uint8, device=dev) if workspace is None else workspace
    _check_tensors('gpp_track_f64', dev, ((out, torch.float32, (N, D, GPP_POSE_COLS)), (ids, torch.int32, (N, D)), (hits, torch.int32, (N, D)),
                                          (state_out, torch.uint8, (S, nbytes))))
    if workspace.dtype != torch.uint8 or workspace.device != dev:
        raise ValueError('gpp_track_f64: the workspace must be uint8 on {}'.format(dev))
    name = 'gpp_track_kf_f64' if kf is not None else 'gpp_track_ego_f64' if ego is not None else 'gpp_track_optimal_f64' if optimal else 'gpp_track_f64'
    fn = _entry(name)
    # the four argument lists of include/gpp.h differ in the middle: the head and the tail are one
    args = [ptr(rows), N, D, seq, S, ptr(state_in), ptr(state_out)]
    if kf is not None:
        args += [ptr(cov_in), ptr(cov_out)]
    args.append(ctypes.byref(params))
    if kf is not None:
        args.append(ctypes.byref(kf))
    if kf is not None or ego is not None:
        args += [None if ego is None else ego.ctypes.data_as(c_void_p), int(bool(optimal))]
    args += [ptr(out), ptr(ids), ptr(hits), ptr(workspace), int(workspace.numel()), stream_ptr()]
    check(fn(*args), name)
    return (out, ids, hits, state_out) if kf is None else (out, ids, hits, state_out, cov_out)


def track_smooth_workspace_bytes(N, n_seg, cells):
    return _bytes('gpp_track_smooth_workspace_bytes', int(N), int(n_seg), int(cells))


def track_smooth(rows, seg_start, seg_frame, cell_row, kf, ego=None, out=None, covariance=True, workspace=None):
    """ gpp_track_smooth_f64 on the current stream: rows (N, D, 36) float32 on the device -- the RAW rows of a finished run --, the index of
    utils/track_smooth.segments_of as HOST NumPy arrays (seg_start (n_seg + 1) int64, seg_frame (n_seg) int32, cell_row (cells) int32), kf
    a TrackKfParams, ego None or the (N, 16) float64 host records -> (rows_out (N, D, 36) float32, row_cov (N, D, 3) float64 or None,
    fill_rows (fills, 36) float32, fill_cov (fills, 3) float64 or None) on the device; one fill per -1 of cell_row, in its order.  out: where
    the rows go (default: a new tensor; `rows` itself: in place); covariance False: neither covariance is asked for.  The entry point
    waits for its copy of the index, not for its launches. """
    import numpy as np
    import torch
    if rows.dim() != 3 or rows.dtype != torch.float32 or rows.shape[2] != GPP_POSE_COLS or not rows.is_contiguous():
        raise ValueError('gpp_track_smooth_f64: rows must be a dense (N, D, {}) float32 tensor, got {} {}'.format(GPP_POSE_COLS, tuple(rows.shape), rows.dtype))
    N, D = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    seg_start, seg_frame = np.ascontiguousarray(seg_start, np.int64), np.ascontiguousarray(seg_frame, np.int32)
    cell_row = np.ascontiguousarray(cell_row, np.int32)
    n_seg = int(seg_frame.shape[0])
    if seg_start.shape != (n_seg + 1,) or cell_row.ndim != 1 or seg_frame.ndim != 1:
        raise ValueError('gpp_track_smooth_f64: seg_start must be (n_seg + 1,), seg_frame (n_seg,), cell_row (cells,); got {} {} {}'.format(
            seg_start.shape, seg_frame.shape, cell_row.shape))
    cells = int(cell_row.shape[0])
    if int(seg_start[-1]) != cells:
        raise ValueError('gpp_track_smooth_f64: seg_start ends at {}, cell_row has {} cells'.format(int(seg_start[-1]), cells))
    fills = int((cell_row < 0).sum())
    if ego is not None:
        ego = np.ascontiguousarray(ego, np.float64)
        if ego.shape != (N, GPP_TRACK_EGO_FIELDS):
            raise ValueError('gpp_track_smooth_f64: ego must be ({}, {}) float64 on the host, got {}'.format(N, GPP_TRACK_EGO_FIELDS, ego.shape))
    out = torch.empty_like(rows) if out is None else out
    _check_tensors('gpp_track_smooth_f64', dev, ((out, torch.float32, (N, D, GPP_POSE_COLS)),), contiguous=True)
    row_cov = torch.empty((N, D, 3), dtype=torch.float64, device=dev) if covariance else None
    fill_rows = torch.empty((fills, GPP_POSE_COLS), dtype=torch.float32, device=dev)
    fill_cov = torch.empty((fills, 3), dtype=torch.float64, device=dev) if covariance else None
    need = track_smooth_workspace_bytes(N, n_seg, cells)
    workspace = torch.empty((max(need, 8),), dtype=torch.uint8, device=dev) if workspace is None else workspace
    if workspace.dtype != torch.uint8 or workspace.device != dev:
        raise ValueError('gpp_track_smooth_f64: the workspace must be uint8 on {}'.format(dev))
    host = lambda a, t: a.ctypes.data_as(_P(t))  # noqa: E731
    check(_entry('gpp_track_smooth_f64')(ptr(rows), N, D, host(seg_start, c_int64), host(seg_frame, ctypes.c_int32), host(cell_row, ctypes.c_int32),
                                         n_seg, ctypes.byref(kf), None if ego is None else ego.ctypes.data_as(c_void_p), ptr(out),
                                         ptr(row_cov), ptr(fill_rows) if fills else None, ptr(fill_cov) if fills else None,
                                         ptr(workspace), int(workspace.numel()), stream_ptr()), 'gpp_track_smooth_f64')
    return out, row_cov, fill_rows, fill_cov


def mot_assign(overlaps, labels, label_counts, rows, ids, params):
    """ gpp_mot_assign on the current stream: overlaps (N, 4, D, A) float64, labels (N, A, 16) float64, label_counts (N,) int32, rows
    (N, D, 36) float32 and ids (N, D) int32 on the device, params a MotParams -> (match (N, A) int32, label_outcome (N, A) int32,
    row_outcome (N, D) int32, frame_counts (N, 8) int64) on the device; no synchronisation """
    import torch
    N, D, A = _kitti_check(rows, labels, label_counts, 'gpp_mot_assign')
    dev = rows.device
    _check_tensors('gpp_mot_assign', dev, ((overlaps, torch.float64, (N, 4, D, A)), (ids, torch.int32, (N, D))))
    match = torch.full((N, A), -1, dtype=torch.int32, device=dev)
    label_outcome = torch.zeros((N, A), dtype=torch.int32, device=dev)
    row_outcome = torch.zeros((N, D), dtype=torch.int32, device=dev)
    frame_counts = torch.zeros((N, GPP_MOT_FRAME_COUNTS), dtype=torch.int64, device=dev)
    check(lib().gpp_mot_assign(ptr(overlaps), ptr(labels), ptr(label_counts), ptr(rows), ptr(ids), N, D, A, ctypes.byref(params),
                               ptr(match), ptr(label_outcome), ptr(row_outcome), ptr(frame_counts), stream_ptr()), 'gpp_mot_assign')
    return match, label_outcome, row_outcome, frame_counts


def mot_clear_workspace_bytes(S):
    return _bytes('gpp_mot_clear_workspace_bytes', int(S))


def mot_clear(match, label_outcome, traj, ids, frame_counts, seq_start, max_traj):
    """ gpp_mot_clear on the current stream: match, label_outcome and traj (N, A) int32, ids (N, D) int32 and frame_counts (N, 8) int64 on
    the device, seq_start (S + 1) host integers -> (seq_counts (S, 16) int64, traj_table (S, max_traj, 4) int32) on the device; no
    synchronisation """
    import torch
    N, A, D = int(match.shape[0]), int(match.shape[1]), int(ids.shape[1])
    dev = match.device
    _check_tensors('gpp_mot_clear', dev, ((match, torch.int32, (N, A)), (label_outcome, torch.int32, (N, A)), (traj, torch.int32, (N, A)),
                                          (ids, torch.int32, (N, D)), (frame_counts, torch.int64, (N, GPP_MOT_FRAME_COUNTS))))
    S = len(seq_start) - 1
    seq = (ctypes.c_int32 * (S + 1))(*[int(v) for v in seq_start])
    seq_counts = torch.zeros((S, GPP_MOT_SEQ_COUNTS), dtype=torch.int64, device=dev)
    traj_table = torch.zeros((S, int(max_traj), GPP_MOT_TRAJ_COLS), dtype=torch.int32, device=dev)
    workspace = torch.empty((mot_clear_workspace_bytes(S),), dtype=torch.uint8, device=dev)
    check(lib().gpp_mot_clear(ptr(match), ptr(label_outcome), ptr(traj), ptr(ids), ptr(frame_counts), N, D, A, seq, S, int(max_traj),
                              ptr(seq_counts), ptr(traj_table), ptr(workspace), int(workspace.numel()), stream_ptr()), 'gpp_mot_clear')
    return seq_counts, traj_table


def _pair_workspace(score):
    """ (SCORE_workspace_bytes, SCORE_workspace) of a score that keeps pair tables (csrc/pair_tables.h), 'hota' or 'idf1' """
    def workspace_bytes(cells, vecs, max_frames, S):
        return _bytes('gpp_{}_workspace_bytes'.format(score), int(cells), int(vecs), int(max_frames), int(S))

    def workspace(cells, vecs, max_frames, S, device):
        """ the zeroed workspace of the score's calls for pair tables of `cells` cells and `vecs` counters in all, up to `max_frames`
        frames a call and S sequences """
        import torch
        return torch.zeros((workspace_bytes(cells, vecs, max_frames, S),), dtype=torch.uint8, device=device)

    return workspace_bytes, workspace


hota_workspace_bytes, hota_workspace = _pair_workspace('hota')
idf1_workspace_bytes, idf1_workspace = _pair_workspace('idf1')


def hota_tables(workspace, cells, vecs):
    """ the views include/gpp.h documents: (P int64 (cells,), A int32 (cells,), hist int32 (cells, 20), counters int32 (vecs,)) """
    import torch
    cells, vecs = int(cells), int(vecs)
    at_hist = (12 * cells + 15) // 16 * 16
    at_cnt = at_hist + 4 * GPP_HOTA_HIST * cells
    return (workspace[:8 * cells].view(torch.int64), workspace[8 * cells:12 * cells].view(torch.int32),
            workspace[at_hist:at_cnt].view(torch.int32).view(cells, GPP_HOTA_HIST), workspace[at_cnt:at_cnt + 4 * vecs].view(torch.int32))


def _host_table(what, table, lines, cols):
    """ a host table of `lines` x `cols` integers as a contiguous int32 array (kept alive by the caller for the call) """
    import numpy as np
    out = np.ascontiguousarray(np.asarray(table).reshape(-1), dtype=np.int32)
    if out.size != lines * cols:
        raise ValueError('{}: the host table must hold {} lines of {}'.format(what, lines, cols))
    return out


def _table_ptr(table):
    return table.ctypes.data_as(_HOST_I32)


def _pair_frames(what, overlaps, label_outcome, row_outcome, traj, trk, frame_tab, workspace):
    """ what the frame calls on pair tables (gpp_hota_potential, gpp_hota_match, gpp_idf1_count) take alike -> (N, D, A, the host table) """
    import torch
    if overlaps.dim() != 4:
        raise ValueError('{}: overlaps must be (N, 4, D, A), got {}'.format(what, tuple(overlaps.shape)))
    N, D, A = int(overlaps.shape[0]), int(overlaps.shape[2]), int(overlaps.shape[3])
    dev = overlaps.device
    _check_tensors(what, dev, ((overlaps, torch.float64, (N, 4, D, A)), (label_outcome, torch.int32, (N, A)), (row_outcome, torch.int32, (N, D)),
                               (traj, torch.int32, (N, A)), (trk, torch.int32, (N, D))))
    if workspace.dtype != torch.uint8 or workspace.device != dev:
        raise ValueError('{}: the workspace must be uint8 on {}'.format(what, dev))
    return N, D, A, _host_table(what, frame_tab, N, GPP_HOTA_TAB_COLS)


def hota_potential(overlaps, label_outcome, row_outcome, traj, trk, metric, frame_tab, cells, vecs, workspace):
    """ gpp_hota_potential on the current stream (pass 1): overlaps (N, 4, D, A) float64, label_outcome and traj (N, A) int32, row_outcome
    and trk (N, D) int32 on the device, frame_tab N * 4 host integers (cell_base, n_gt, n_trk, vec_base per frame), the workspace of
    hota_workspace -- adds the frames to the pair tables in the workspace; no synchronisation """
    N, D, A, tab = _pair_frames('gpp_hota_potential', overlaps, label_outcome, row_outcome, traj, trk, frame_tab, workspace)
    check(lib().gpp_hota_potential(ptr(overlaps), ptr(label_outcome), ptr(row_outcome), ptr(traj), ptr(trk), N, D, A, int(metric), _table_ptr(tab),
                                   int(cells), int(vecs), ptr(workspace), int(workspace.numel()), stream_ptr()), 'gpp_hota_potential')


def hota_match(overlaps, label_outcome, row_outcome, traj, trk, metric, frame_tab, cells, vecs, workspace):
    """ gpp_hota_match on the current stream (pass 2, after pass 1 has seen every frame of the sequences): the arguments of hota_potential
    -> (hota_match (N, A) int32, frame_hota (N, 40) int64) on the device; no synchronisation """
    import torch
    N, D, A, tab = _pair_frames('gpp_hota_match', overlaps, label_outcome, row_outcome, traj, trk, frame_tab, workspace)
    match = torch.full((N, A), -1, dtype=torch.int32, device=overlaps.device)
    frame_hota = torch.zeros((N, GPP_HOTA_FRAME_COLS), dtype=torch.int64, device=overlaps.device)
    check(lib().gpp_hota_match(ptr(overlaps), ptr(label_outcome), ptr(row_outcome), ptr(traj), ptr(trk), N, D, A, int(metric), _table_ptr(tab),
                               int(cells), int(vecs), ptr(match), ptr(frame_hota), ptr(workspace), int(workspace.numel()), stream_ptr()),
          'gpp_hota_match')
    return match, frame_hota


def hota_reduce(frame_hota, seq_tab, cells, vecs, workspace):
    """ gpp_hota_reduce on the current stream: frame_hota (N, 40) int64 on the device, seq_tab S * 6 host integers (cell_base, n_gt, n_trk,
    vec_base, first frame, one past the last) -> seq_hota (S, 19, 8) int64 on the device: TP FN FP SQ ASS ASSRE ASSPR 0; no synchronisation """
    import torch
    if frame_hota.dim() != 2 or frame_hota.dtype != torch.int64 or int(frame_hota.shape[1]) != GPP_HOTA_FRAME_COLS:
        raise ValueError('gpp_hota_reduce: frame_hota must be (N, {}) int64, got {} {}'.format(GPP_HOTA_FRAME_COLS, tuple(frame_hota.shape), frame_hota.dtype))
    S = len(seq_tab) // GPP_HOTA_SEQ_TAB_COLS
    tab = _host_table('gpp_hota_reduce', seq_tab, S, GPP_HOTA_SEQ_TAB_COLS)
    seq_hota = torch.zeros((S, GPP_HOTA_LEVELS, GPP_HOTA_SEQ_COLS), dtype=torch.int64, device=frame_hota.device)
    check(lib().gpp_hota_reduce(ptr(frame_hota), int(frame_hota.shape[0]), _table_ptr(tab), S, int(cells), int(vecs), ptr(seq_hota), ptr(workspace),
                                int(workspace.numel()), stream_ptr()), 'gpp_hota_reduce')
    return seq_hota


def idf1_tables(workspace, cells, vecs):
    """ the views include/gpp.h documents, to read and to write: (C int32 (cells,), counters int32 (vecs,)) """
    import torch
    cells, vecs = int(cells), int(vecs)
    at_cnt = (4 * cells + 15) // 16 * 16
    return workspace[:4 * cells].view(torch.int32), workspace[at_cnt:at_cnt + 4 * vecs].view(torch.int32)


def idf1_count(overlaps, label_outcome, row_outcome, traj, trk, metric, frame_tab, cells, vecs, workspace):
    """ gpp_idf1_count on the current stream (pass 1): the arguments of hota_potential, the workspace of idf1_workspace -- adds the frames
    to the table C and to the counters in the workspace; no synchronisation """
    N, D, A, tab = _pair_frames('gpp_idf1_count', overlaps, label_outcome, row_outcome, traj, trk, frame_tab, workspace)
    check(lib().gpp_idf1_count(ptr(overlaps), ptr(label_outcome), ptr(row_outcome), ptr(traj), ptr(trk), N, D, A, int(metric), _table_ptr(tab),
                               int(cells), int(vecs), ptr(workspace), int(workspace.numel()), stream_ptr()), 'gpp_idf1_count')


def idf1_assign(seq_tab, cells, vecs, workspace):
    """ gpp_idf1_assign on the current stream (pass 2, after pass 1 has seen every frame): seq_tab S * 6 host integers (cell_base, n_gt,
    n_trk, vec_base, and two that are not read) -> (id_match (vecs,) int32: trajectory g of a sequence at vec_base + g, -1 elsewhere,
    seq_idf1 (S, 8) int64: IDTP IDFN IDFP sum-gc sum-tc cost G T) on the device; no synchronisation """
    import torch
    if workspace.dtype != torch.uint8 or not workspace.is_cuda:
        raise ValueError('gpp_idf1_assign: the workspace must be uint8 on the device')
    S = len(seq_tab) // GPP_HOTA_SEQ_TAB_COLS
    tab = _host_table('gpp_idf1_assign', seq_tab, S, GPP_HOTA_SEQ_TAB_COLS)
    id_match = torch.full((max(int(vecs), 1),), -1, dtype=torch.int32, device=workspace.device)[:int(vecs)]
    seq_idf1 = torch.zeros((S, GPP_IDF1_SEQ_COLS), dtype=torch.int64, device=workspace.device)
    check(lib().gpp_idf1_assign(_table_ptr(tab), S, int(cells), int(vecs), ptr(id_match), ptr(seq_idf1), ptr(workspace), int(workspace.numel()),
                                stream_ptr()), 'gpp_idf1_assign')
    return id_match, seq_idf1


def label_prep(labels, label_counts, P, trig, det_types=0, own_box=True, detections=True):
    """ gpp_label_prep_f64 on the current stream: labels (B, A, 16) float64, label_counts (B,) int32, P (B, 3, 4) float64 and trig (B, A, 2)
    float64 (cos, sin of r_y, computed on the host) on the device -> (mod (B, A, 20) float64, and with `detections` the five arrays of the
    decode's layout: boxes (B, A, 12), dims (B, A, 3), scores (B, A) float32, labels (B, A), orientations (B, A) int32 -- else None);
    everything stays on the device, no synchronisation """
    import torch
    if labels.dim() != 3:
        raise ValueError('gpp_label_prep_f64: labels must be (B, A, {}), got {}'.format(GPP_KITTI_LABEL_COLS, tuple(labels.shape)))
    B, A = int(labels.shape[0]), int(labels.shape[1])
    dev = labels.device
    _check_tensors('gpp_label_prep_f64', dev, ((labels, torch.float64, (B, A, GPP_KITTI_LABEL_COLS)), (label_counts, torch.int32, (B,)),
                                               (P, torch.float64, (B, 3, 4)), (trig, torch.float64, (B, A, 2))))
    mod = torch.empty((B, A, GPP_LABEL_MOD_COLS), dtype=torch.float64, device=dev)
    det = None
    if detections:
        det = (torch.empty((B, A, 12), dtype=torch.float32, device=dev), torch.empty((B, A, 3), dtype=torch.float32, device=dev),
               torch.empty((B, A), dtype=torch.float32, device=dev), torch.empty((B, A), dtype=torch.int32, device=dev),
               torch.empty((B, A), dtype=torch.int32, device=dev))
    outs = [ptr(t) for t in det] if detections else [None] * 5
    check(lib().gpp_label_prep_f64(ptr(labels), ptr(label_counts), ptr(P), ptr(trig), B, A, int(det_types), int(bool(own_box)), ptr(mod),
                                   *(outs + [stream_ptr()])), 'gpp_label_prep_f64')
    return mod, det


def table_pitch(M):
    """ the smallest row pitch gpp_poll_costs_u16 and gpp_plane_select take for M planes: M rounded up to 8 (16 bytes) """
    return max(8, (int(M) + 7) // 8 * 8)


def poll_costs(boxes, dims, orient, P_inv, planes, table, row_index=None, row_offset=0, thr=0.7):
    """ gpp_poll_costs_u16 on the current stream: boxes (B, D, 12), dims (B, D, 3) float32, orient (B, D) int32, P_inv (B, 4, 3) float32 and
    planes (M, 4) float32 on the device; row_index (O,) int32 flat rows b * D + d, None = all B * D.  Fills the columns [0, M) of the rows
    [row_offset, row_offset + O) of `table`, a (rows, pitch) int16 tensor that holds the uint16 keys (view it as uint16 on the host).
    No synchronisation; returns O """
    import torch
    if boxes.dim() != 3 or planes.dim() != 2 or table.dim() != 2:
        raise ValueError('gpp_poll_costs_u16: boxes must be (B, D, 12), planes (M, 4) and table (rows, pitch), got {} {} {}'.format(
            tuple(boxes.shape), tuple(planes.shape), tuple(table.shape)))
    B, D, M = int(boxes.shape[0]), int(boxes.shape[1]), int(planes.shape[0])
    want = [(boxes, torch.float32, (B, D, 12)), (dims, torch.float32, (B, D, 3)), (orient, torch.int32, (B, D)), (P_inv, torch.float32, (B, 4, 3)),
            (planes, torch.float32, (M, 4)), (table, torch.int16, tuple(table.shape))]
    O = B * D
    if row_index is not None:
        O = int(row_index.numel())
        want.append((row_index, torch.int32, (O,)))
    _check_tensors('gpp_poll_costs_u16', boxes.device, want)
    rows, pitch = int(table.shape[0]), int(table.shape[1])
    if int(row_offset) < 0 or int(row_offset) + O > rows or pitch < M or pitch % 8:
        raise ValueError('gpp_poll_costs_u16: rows [{}, {}) of {} planes do not fit a table of {} rows, pitch {} (pitch >= M, a multiple of 8)'.format(
            int(row_offset), int(row_offset) + O, M, rows, pitch))
    workspace = torch.empty((max(_bytes('gpp_poll_costs_workspace_bytes', M), 16),), dtype=torch.uint8, device=boxes.device)
    check(lib().gpp_poll_costs_u16(ptr(boxes), ptr(dims), ptr(orient), ptr(P_inv), ptr(planes), B, D, M, float(thr), ptr(row_index), O,
                                   ptr(table), pitch, int(row_offset), ptr(workspace), workspace.numel(), stream_ptr()), 'gpp_poll_costs_u16')
    return O


def plane_select(table, M, K):
    """ gpp_plane_select on the current stream: table (O, pitch) int16 on the device (uint16 keys), its first M columns the planes, K picks ->
    (chosen (K,) int32, trace (K + 1,) int64, best (O,) int16 holding uint16 keys, count (1,) int32) on the device; no synchronisation """
    import torch
    if table.dim() != 2 or table.dtype != torch.int16:
        raise ValueError('gpp_plane_select: table must be (O, pitch) int16, got {} {}'.format(tuple(table.shape), table.dtype))
    O, pitch, M, K = int(table.shape[0]), int(table.shape[1]), int(M), int(K)
    if O < 1 or M < 1 or pitch < M or pitch % 8 or K < 1 or K > M:
        raise ValueError('gpp_plane_select: O = {}, M = {}, pitch = {}, K = {}: needs O >= 1, 1 <= K <= M <= pitch, pitch a multiple of 8'.format(O, M, pitch, K))
    dev = table.device
    chosen = torch.empty((K,), dtype=torch.int32, device=dev)
    trace = torch.empty((K + 1,), dtype=torch.int64, device=dev)
    best = torch.empty((O,), dtype=torch.int16, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    workspace = torch.empty((_bytes('gpp_plane_select_workspace_bytes', M),), dtype=torch.uint8, device=dev)
    check(lib().gpp_plane_select(ptr(table), O, M, pitch, K, ptr(chosen), ptr(trace), ptr(best), ptr(count), ptr(workspace), workspace.numel(),
                                 stream_ptr()), 'gpp_plane_select')
    return chosen, trace, best, count


def pose_costs(boxes, dims, orient, P_inv, want, planes, keys, errs, row_index=None, row_offset=0, thr=0.7):
    """ gpp_pose_costs_u16 on the current stream: the arguments of poll_costs, with want (B, D, 3) float32 (the labels' locations) and two
    tables of one shape, (rows, pitch) int16: `keys` gets what poll_costs writes, `errs` the location error of every pair in 1/256 m
    (65535 where the key is).  No synchronisation; returns O """
    import torch
    if boxes.dim() != 3 or planes.dim() != 2 or keys.dim() != 2:
        raise ValueError('gpp_pose_costs_u16: boxes must be (B, D, 12), planes (M, 4) and keys (rows, pitch), got {} {} {}'.format(
            tuple(boxes.shape), tuple(planes.shape), tuple(keys.shape)))
    B, D, M = int(boxes.shape[0]), int(boxes.shape[1]), int(planes.shape[0])
    expect = [(boxes, torch.float32, (B, D, 12)), (dims, torch.float32, (B, D, 3)), (orient, torch.int32, (B, D)), (P_inv, torch.float32, (B, 4, 3)),
              (want, torch.float32, (B, D, 3)), (planes, torch.float32, (M, 4)), (keys, torch.int16, tuple(keys.shape)),
              (errs, torch.int16, tuple(keys.shape))]
    O = B * D
    if row_index is not None:
        O = int(row_index.numel())
        expect.append((row_index, torch.int32, (O,)))
    _check_tensors('gpp_pose_costs_u16', boxes.device, expect, contiguous=True)
    rows, pitch = int(keys.shape[0]), int(keys.shape[1])
    if int(row_offset) < 0 or int(row_offset) + O > rows or pitch < M or pitch % 8:
        raise ValueError('gpp_pose_costs_u16: rows [{}, {}) of {} planes do not fit tables of {} rows, pitch {} (pitch >= M, a multiple of 8)'.format(
            int(row_offset), int(row_offset) + O, M, rows, pitch))
    workspace = torch.empty((max(_bytes('gpp_poll_costs_workspace_bytes', M), 16),), dtype=torch.uint8, device=boxes.device)
    check(lib().gpp_pose_costs_u16(ptr(boxes), ptr(dims), ptr(orient), ptr(P_inv), ptr(want), ptr(planes), B, D, M, float(thr), ptr(row_index), O,
                                   ptr(keys), ptr(errs), pitch, int(row_offset), ptr(workspace), workspace.numel(), stream_ptr()), 'gpp_pose_costs_u16')
    return O


def plane_select_polled(keys, errs, M, K):
    """ gpp_plane_select_polled on the current stream: keys and errs (O, pitch) int16 on the device (uint16 values), their first M columns
    the planes, K picks -> (chosen (K,) int32, trace (K + 1,) int64, best (O,), cur (O,) int16 holding uint16 values, count (1,) int32) on
    the device; no synchronisation """
    import torch
    if keys.dim() != 2:
        raise ValueError('gpp_plane_select_polled: keys and errs must be (O, pitch), got {} and {}'.format(tuple(keys.shape), tuple(errs.shape)))
    _check_tensors('gpp_plane_select_polled', keys.device, ((keys, torch.int16, tuple(keys.shape)), (errs, torch.int16, tuple(keys.shape))),
                   contiguous=True)
    O, pitch, M, K = int(keys.shape[0]), int(keys.shape[1]), int(M), int(K)
    if O < 1 or M < 1 or pitch < M or pitch % 8 or K < 1 or K > M:
        raise ValueError('gpp_plane_select_polled: O = {}, M = {}, pitch = {}, K = {}: needs O >= 1, 1 <= K <= M <= pitch, pitch a multiple of 8'.format(O, M, pitch, K))
    dev = keys.device
    chosen = torch.empty((K,), dtype=torch.int32, device=dev)
    trace = torch.empty((K + 1,), dtype=torch.int64, device=dev)
    best = torch.empty((O,), dtype=torch.int16, device=dev)
    cur = torch.empty((O,), dtype=torch.int16, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    workspace = torch.empty((_bytes('gpp_plane_select_polled_workspace_bytes', M),), dtype=torch.uint8, device=dev)
    check(lib().gpp_plane_select_polled(ptr(keys), ptr(errs), O, M, pitch, K, ptr(chosen), ptr(trace), ptr(best), ptr(cur), ptr(count), ptr(workspace),
                                        workspace.numel(), stream_ptr()), 'gpp_plane_select_polled')
    return chosen, trace, best, cur, count


def road_points(points, offsets, T, max_points, region_q):
    """ gpp_road_points_i32 on the current stream: points (total, 4) float32, offsets (F + 1) int32 and T (F, 12) float64 on the device,
    max_points >= every frame's size, region_q = (xq, yq, zq) in quanta -> (q (total, 3) int32, kept (F,) int32) on the device; the rows of
    q past a frame's kept count are zero.  No synchronisation """
    import torch
    if points.dim() != 2 or offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError('gpp_road_points_i32: points must be (total, 4) and offsets (F + 1,), got {} {}'.format(tuple(points.shape), tuple(offsets.shape)))
    total, F = int(points.shape[0]), int(offsets.numel()) - 1
    _check_tensors('gpp_road_points_i32', points.device, ((points, torch.float32, (total, 4)), (offsets, torch.int32, (F + 1,)), (T, torch.float64, (F, 12))))
    q = torch.zeros((total, 3), dtype=torch.int32, device=points.device)
    kept = torch.zeros((F,), dtype=torch.int32, device=points.device)
    xq, yq, zq = [int(v) for v in region_q]
    check(lib().gpp_road_points_i32(ptr(points), ptr(offsets), ptr(T), F, total, int(max_points), xq, yq, zq, ptr(q), ptr(kept), stream_ptr()),
          'gpp_road_points_i32')
    return q, kept


def road_score(q, offsets, kept, frame_id, seed, max_points, H, c2, hlo2, hhi2, tq2):
    """ gpp_road_score on the current stream: q (total, 3) int32, offsets (F + 1,), kept (F,) int32 and frame_id (F,) int32 holding the uint32
    ids, on the device -> count (F, H) int32 on the device (-1 = an invalid hypothesis); no synchronisation """
    import torch
    total, F, H = int(q.shape[0]), int(kept.numel()), int(H)
    _check_tensors('gpp_road_score', q.device, ((q, torch.int32, (total, 3)), (offsets, torch.int32, (F + 1,)), (kept, torch.int32, (F,)),
                                                (frame_id, torch.int32, (F,))))
    count = torch.empty((F, max(H, 0)), dtype=torch.int32, device=q.device)
    check(lib().gpp_road_score(ptr(q), ptr(offsets), ptr(kept), ptr(frame_id), int(seed) & 0xffffffff, F, total, int(max_points), H,
                               float(c2), float(hlo2), float(hhi2), float(tq2), ptr(count), stream_ptr()), 'gpp_road_score')
    return count


def road_winner(count, min_inliers):
    """ gpp_road_winner on the current stream: count (F, H) int32 on the device -> (winner (F,) int32, -1 = no plane; inliers (F,) int32) """
    import torch
    if count.dim() != 2 or count.dtype != torch.int32:
        raise ValueError('gpp_road_winner: count must be (F, H) int32, got {} {}'.format(tuple(count.shape), count.dtype))
    F, H = int(count.shape[0]), int(count.shape[1])
    winner = torch.full((F,), -1, dtype=torch.int32, device=count.device)
    inliers = torch.zeros((F,), dtype=torch.int32, device=count.device)
    check(lib().gpp_road_winner(ptr(count), F, H, int(min_inliers), ptr(winner), ptr(inliers), stream_ptr()), 'gpp_road_winner')
    return winner, inliers


def road_moments(q, offsets, kept, frame_id, seed, winner, max_points, H, tq2):
    """ gpp_road_moments on the current stream -> sums (F, 10) int64 on the device: N, Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, Szy, Syy over the
    winner's inliers, zero for a frame without a winner; no synchronisation """
    import torch
    total, F = int(q.shape[0]), int(kept.numel())
    _check_tensors('gpp_road_moments', q.device, ((q, torch.int32, (total, 3)), (offsets, torch.int32, (F + 1,)), (kept, torch.int32, (F,)),
                                                  (frame_id, torch.int32, (F,)), (winner, torch.int32, (F,))))
    sums = torch.zeros((F, 10), dtype=torch.int64, device=q.device)
    check(lib().gpp_road_moments(ptr(q), ptr(offsets), ptr(kept), ptr(frame_id), int(seed) & 0xffffffff, ptr(winner), F, total, int(max_points),
                                 int(H), float(tq2), ptr(sums), stream_ptr()), 'gpp_road_moments')
    return sums


def road_peel(q, offsets, kept, frame_id, seed, winner, max_points, H, tq2):
    """ gpp_road_peel_i32 on the current stream: the kept points of every frame that are no inliers of `winner`'s plane under `seed`, in
    their order -> (q_out (total, 3) int32, a frame's survivors at the head of its own segment and zeros behind; kept_out (F,) int32) on
    the device, a frame without a winner: kept_out 0.  q is not changed.  No synchronisation """
    import torch
    peel = _entry('gpp_road_peel_i32')
    total, F = int(q.shape[0]), int(kept.numel())
    _check_tensors('gpp_road_peel_i32', q.device, ((q, torch.int32, (total, 3)), (offsets, torch.int32, (F + 1,)), (kept, torch.int32, (F,)),
                                                   (frame_id, torch.int32, (F,)), (winner, torch.int32, (F,))))
    q_out = torch.zeros((total, 3), dtype=torch.int32, device=q.device)
    kept_out = torch.zeros((F,), dtype=torch.int32, device=q.device)
    workspace = torch.empty((_bytes('gpp_road_peel_workspace_bytes', F, int(max_points)),), dtype=torch.uint8, device=q.device)
    check(peel(ptr(q), ptr(offsets), ptr(kept), ptr(frame_id), int(seed) & 0xffffffff, ptr(winner), F, total, int(max_points), int(H), float(tq2),
               ptr(q_out), ptr(kept_out), ptr(workspace), workspace.numel(), stream_ptr()), 'gpp_road_peel_i32')
    return q_out, kept_out


def channel_absmax(buf, M, C, pitch, c_off, layout, out, stream=None):
    """ gpp_channel_absmax on M pixels of a device tensor (pixel m at element m * pitch, channels [c_off, c_off + C)) into the uint32
    table `out` (an int32 tensor of >= C words, cleared by the caller: gpp_absmax_clear) """
    d = AbsmaxDesc(buf.data_ptr(), out.data_ptr(), M, pitch, C, c_off, layout, 0)
    check(lib().gpp_channel_absmax(ctypes.byref(d), stream or stream_ptr()), 'gpp_channel_absmax')


def pack_stem_weights_x3(kernel_147x64, device):
    """ [147][64] float32 folded stem kernel -> device blob of the x3 MFMA stem: [whi 64 x 232 f16][wlo 64 x 232 f16][64 float32 out_scale] """
    import numpy as np
    import torch
    src = np.ascontiguousarray(kernel_147x64, dtype=np.float32)
    dst = np.zeros((2 * 64 * 232 * 2 + 64 * 4,), dtype=np.uint8)
    check(lib().gpp_stem_pack_weights_f16x3(src.ctypes.data_as(c_void_p), dst.ctypes.data_as(c_void_p), dst.nbytes), 'gpp_stem_pack_weights_f16x3')
    return torch.as_tensor(dst).to(device).contiguous()


def pack_stem_weights(kernel_147x64, device):
    """ [147][64] float32 folded stem kernel -> device tensor holding the [64][232] f16 image of the MFMA stem """
    import numpy as np
    import torch
    src = np.ascontiguousarray(kernel_147x64, dtype=np.float32)
    dst = np.zeros((64, 232), dtype=np.float16)
    check(lib().gpp_stem_pack_weights_f16(src.ctypes.data_as(c_void_p), dst.ctypes.data_as(c_void_p), dst.nbytes), 'gpp_stem_pack_weights_f16')
    return torch.as_tensor(dst).to(device).contiguous()
