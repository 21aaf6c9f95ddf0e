"""
What a plan is: the ctypes mirrors of the descriptors of include/gpp.h (gpp_stem_desc ... gpp_plan_op), the op codes and flag bits of
gpp_plan_op.kind, the plan switches, and the Plan a model records for one (batch, H, W, N planes) -- its buffers, descriptors and op
array, who reads and writes what, and the race check over them -- with the pure rules that name the form of a bottleneck and of the head
layers (block_form, head_forms) and the host side of the range audit's table.  models/builder.py builds plans out of these, models/tuning.py
chooses their tiles, models/retinanet.py runs them; nothing here launches a network.
"""

import collections
import ctypes
import os

import numpy as np

from ..backend import hip
from ..layers import conv as C


class StemDesc(ctypes.Structure):
    _fields_ = [('inp', ctypes.c_void_p), ('weight', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('out', ctypes.c_void_p),
                ('dtype', ctypes.c_int32), ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('range_counter', ctypes.c_void_p)]


class PoolDesc(ctypes.Structure):
    _fields_ = [('inp', ctypes.c_void_p), ('out', ctypes.c_void_p), ('dtype', ctypes.c_int32), ('B', ctypes.c_int32),
                ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('C', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class RaggedStemDesc(ctypes.Structure):
    """ gpp_ragged_stem_desc (include/gpp.h): the stem of a batch of one height class; H of `stem` = the 4 Hp rows of the canvas """
    _fields_ = [('stem', StemDesc), ('heights', ctypes.c_void_p), ('Hp', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class RaggedPoolDesc(ctypes.Structure):
    """ gpp_ragged_pool_desc (include/gpp.h): pool1 behind a ragged stem; H of `pool` = the 2 Hp rows of the stored conv map """
    _fields_ = [('pool', PoolDesc), ('heights', ctypes.c_void_p), ('Hp', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class ReluDesc(ctypes.Structure):
    _fields_ = [('inp', ctypes.c_void_p), ('out', ctypes.c_void_p), ('in_bstride', ctypes.c_int64),
                ('out_bstride', ctypes.c_int64), ('count', ctypes.c_int64), ('dtype', ctypes.c_int32), ('B', ctypes.c_int32)]


class DetectDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('cls_logits', 'regression', 'regression_dim', 'anchors', 'boxes', 'dims',
                                               'scores', 'labels', 'orientations', 'anchor_index', 'counts', 'workspace')] + \
               [('workspace_bytes', ctypes.c_size_t), ('n_anchors', ctypes.c_int64),
                ('B', ctypes.c_int32), ('num_base_anchors', ctypes.c_int32), ('fused_layout', ctypes.c_int32),
                ('max_det', ctypes.c_int32), ('score_thr', ctypes.c_float), ('iou_thr', ctypes.c_float)]


class CandidatePixelsDesc(ctypes.Structure):
    """ gpp_candidate_pixels_desc (include/gpp.h): the candidate pass of a DetectDesc, then the pixel lists of the gathered head output layers """
    _fields_ = [('detect', ctypes.c_void_p), ('lists', hip.PixelListDesc)]


class PollDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('boxes', 'dims', 'orient', 'P_inv', 'planes', 'keypoints', 'keyplanes',
                                               'residuals', 'best_idx', 'workspace')] + \
               [('workspace_bytes', ctypes.c_size_t), ('B', ctypes.c_int32), ('D', ctypes.c_int32), ('N', ctypes.c_int32),
                ('planes_batched', ctypes.c_int32), ('thr', ctypes.c_float), ('reserved', ctypes.c_int32)]


class PoseDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('boxes', 'dims', 'scores', 'labels', 'orientations', 'keypoints', 'residuals',
                                               'frame_info', 'rows', 'counts')] + \
               [('B', ctypes.c_int32), ('D', ctypes.c_int32), ('score_thr', ctypes.c_float), ('reserved', ctypes.c_int32)]


class CuboidNmsDesc(ctypes.Structure):
    _fields_ = [('rows', ctypes.c_void_p), ('counts', ctypes.c_void_p), ('suppressor', ctypes.c_void_p), ('iou_thr', ctypes.c_double),
                ('B', ctypes.c_int32), ('D', ctypes.c_int32), ('metric', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class PreactDesc(ctypes.Structure):
    _fields_ = [('conv', ctypes.c_void_p), ('in_scale', ctypes.c_void_p), ('in_shift', ctypes.c_void_p)]


class DensePoolDesc(ctypes.Structure):
    _fields_ = [('inp', ctypes.c_void_p), ('out', ctypes.c_void_p), ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('W', ctypes.c_int32),
                ('C', ctypes.c_int32), ('pad', ctypes.c_int32), ('out_pitch', ctypes.c_int32)]


class PlanOp(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('tag', ctypes.c_int32), ('desc', ctypes.c_void_p)]


class TailDesc(ctypes.Structure):
    _fields_ = [('conv3x3', ctypes.c_void_p), ('conv1x1', ctypes.c_void_p), ('tile_rows', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class BlockDesc(ctypes.Structure):
    _fields_ = [('conv1x1_a', ctypes.c_void_p), ('conv3x3_b', ctypes.c_void_p), ('conv1x1_c', ctypes.c_void_p), ('tile', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class BlockProjDesc(ctypes.Structure):         # gpp_block_proj_desc: a BlockDesc whose `reserved` (the header's `form`) is 1, then the shortcut's layer
    _fields_ = [('conv1x1_a', ctypes.c_void_p), ('conv3x3_b', ctypes.c_void_p), ('conv1x1_c', ctypes.c_void_p), ('tile', ctypes.c_int32),
                ('form', ctypes.c_int32), ('conv1x1_proj', ctypes.c_void_p)]


OP_STEM, OP_MAXPOOL, OP_CONV, OP_RELU, OP_DETECT, OP_POLL, OP_TAIL = 1, 2, 3, 4, 5, 6, 7
OP_BLOCK = 16
OP_DETECT_CANDIDATES, OP_DETECT_SELECT, OP_DETECT_EMIT = 8, 9, 10
OP_DETECT_OSF = 12
OP_STEM_POOL = 13
OP_MAXPOOL_PAD, OP_AVGPOOL, OP_CONV_PREACT = 17, 18, 32         # DenseNet (include/gpp.h)
OP_MOBILENET_STEM, OP_MOBILENET_BLOCK = 33, 34                  # MobileNet (include/gpp.h)
OP_POSE = 19                                                    # RetinaNet3D(pose=True): gpp_pose_f32 behind the polling
OP_CUBOID_NMS = 20                                              # RetinaNet3D(pose=True, cuboid_nms=(metric, threshold)): gpp_cuboid_nms_f64 behind the pose stage
OP_ABSMAX, OP_ABSMAX_CLEAR = 35, 36                             # RetinaNet3D(range_audit=True): gpp_channel_absmax behind every audited map
OP_STEM_RAGGED, OP_STEM_POOL_RAGGED, OP_MAXPOOL_RAGGED = 37, 38, 39    # ragged plans (plan_for(..., ragged=True)): per-image heights from a device table
OP_DETECT_CANDIDATE_PIXELS = 40                                 # OP_DETECT_CANDIDATES + gpp_detect_pixel_lists (sparse head outputs)
DETECT_OPS = (OP_DETECT, OP_DETECT_CANDIDATES, OP_DETECT_SELECT, OP_DETECT_EMIT, 12, OP_DETECT_CANDIDATE_PIXELS)
OP_JOIN, OP_SYNC = 0x10000, 0x20000


# the effective plan switches of one (model, batch), read from the GPP_* variables by plan_options (RetinaNet3D._plan_options)
PlanOptions = collections.namedtuple('PlanOptions', 'x3_level fuse_stem_pool stage_chunks half_stages fuse_tail fuse_block fuse_block_proj '
                                                    'fuse_block_inproj fuse_inproj_rounds '
                                                    'br1_lane fpn_lanes p4_lane head_lanes decode_overlap cls_lane autotune tune_key sparse_heads '
                                                    'sparse_tower sparse_tower_rounds sparse_deep sparse_deep_rounds sparse_depth')


def plan_options(model, B):
    """ every GPP_* switch of the plan builder, read once per plan (when its PlanBuilder is made), as its effective value for this model
    and batch (PlanOptions) """
    env = os.environ.get
    x3 = model.dtype in C.X3_TYPES
    # x3 types: maps written and read by convolutions only are stored PRE-SPLIT ([32 hi | 32 lo] halves per 32 channels,
    # gpp_conv_desc.x3_split): GPP_X3_SPLIT=2 (default) every such map, 1 = only the maps between the FPN / head layers -- 80 % of the
    # FLOPs, all of them matrix-pipe bound -- 0 = none.  Written that way by the producing layer's epilogue, read by the consumers
    # without the per-fragment split on the vector ALU.
    x3_split = env('GPP_X3_SPLIT', '2')
    x3_level = int(x3_split) if x3 else 0
    # GPP_STAGE_CHUNKS="2,4,8,8": a stage chunk of images by chunk of images, to keep a chunk's working set inside the 256 MiB Infinity
    # Cache; measured on MI355X at B = 8 this LOSES 1-6 % (the smaller launches cost more than the on-die re-reads save): off
    chunks = env('GPP_STAGE_CHUNKS')
    # GPP_FUSE_TAIL: widths whose branch2b + branch2c run as one launch ("" or 0 for none).  Measured at B = 8, same box, whole step:
    # none 1553, res3 only 1562, res2 + res3 1571 images/s (in isolation the fused res2 launch is no faster than its two layers --
    # 122 us vs 36 + 80 -- but the step is: 69 MB less through HBM per block).  The x3 form (bottleneck_tail_x3_kernel) reads
    # pre-split maps at C = 64 (res2) only -- at C = 128 its LDS footprint leaves one workgroup per CU; float32 operands: none
    tail_widths = env('GPP_FUSE_TAIL', '64,128')
    fuse_tail = [int(v) for v in tail_widths.split(',') if v.strip() and int(v) > 0]
    if x3:
        fuse_tail = [v for v in fuse_tail if v == 64] if x3_level >= 2 else []
    elif model.esz == 4:
        fuse_tail = []
    # GPP_FUSE_BLOCK: widths whose IDENTITY blocks (branch2a + 2b + 2c + shortcut) run as one launch (gpp_bottleneck_block; x3 types on
    # pre-split maps): res2 (C = 64: 4-wavefront workgroups, two per CU; x in once, y out once: 245 -> 212 us per block at B = 8) and
    # res3 (C = 128: 8 wavefronts, one per CU; at parity with its three launches in isolation, half their fabric bytes).  Same-box A/B
    # of the step (profiles/r6/ab_fuse_block_*.txt): B = 8: 780 -> 793 images/s (+1.7 %) with both, +0.9 % with res2 alone; B = 4
    # +1.2 %, B = 2 +0.7 %, batch-1 plan 2.67 -> 2.65 ms.  "" for the separate launches (bit-identical either way).  Projection
    # blocks too (GPP_FUSE_BLOCK_PROJ=1) measured -0.6 %: off.
    block_widths = env('GPP_FUSE_BLOCK', '64,128')
    fuse_block = [int(v) for v in block_widths.split(',') if v.strip()] if (x3 and x3_level >= 2) else []
    if model.audit:
        # an audit plan reads every operand map in HBM: the separate launches wherever a fused form keeps one in LDS (bit-identical
        # to them: tests/test_block_gpu.py), so the results do not change
        fuse_tail, fuse_block = [], []
    # GPP_FUSE_BLOCK_INPROJ (default 1; with 64 in GPP_FUSE_BLOCK): res2a -- the stride-1 projection block -- as ONE launch that computes the
    # shortcut itself (gpp_bottleneck_block_proj): no res2a_branch1 launch, no shortcut map through HBM (276 MB written and read back at
    # B = 8).  Only where a batch part's launch fields more than GPP_FUSE_INPROJ_MIN_ROUNDS rounds of 2 x 256 workgroups of 8 x 14 pixels
    # (a rule of layer, map size and batch part); 0 = res2a as three launches.  Bit-identical either way.
    inproj = env('GPP_FUSE_BLOCK_INPROJ', '1') != '0'
    head_lanes = env('GPP_HEAD_LANES', '0') != '0'
    fpn_lanes = head_lanes or env('GPP_FPN_LANES', '1') != '0'
    overlap = env('GPP_DECODE_OVERLAP', '1') != '0' and not head_lanes and not model.osf
    sparse = overlap and not model.audit and env('GPP_SPARSE_HEADS', '1') != '0'
    return PlanOptions(
        x3_level=x3_level,
        fuse_stem_pool=not model.densenet and not model.mobilenet and (model.esz == 2 or model.stem_x3) and env('GPP_FUSE_STEM_POOL', '1') != '0',
        stage_chunks=tuple(max(1, min(B, int(v))) for v in chunks.split(',')) if chunks else (B,) * 4,
        # GPP_HALF_LANES (default "0,1,2,3" = res2 .. res5; "" for whole batches): a launch of these stages fills the 256 CUs 0.7 - 1.4
        # times and is bound by tile fills and first-touch latency; two half-batch chains in flight overlap one's prologue / epilogue /
        # barrier waits with the other's main loop (f16x3 step, same box: 775 -> 793 images/s; three parts: 801 against 811).  res2
        # since round 6, with fused identity blocks: B = 8 +0.7 %, B = 4 +1.1 %, B = 2 +1.1 % (profiles/r6/ab_half_lanes_with_blocks.txt)
        half_stages=frozenset(int(v) for v in env('GPP_HALF_LANES', '0,1,2,3').split(',') if v.strip()) if B >= 2 else frozenset(),
        fuse_tail=tuple(v for v in fuse_tail if v in (64, 128)),
        fuse_block=tuple(v for v in fuse_block if v in (64, 128)),
        fuse_block_proj=env('GPP_FUSE_BLOCK_PROJ', '0') != '0',
        fuse_block_inproj=inproj,
        fuse_inproj_rounds=float(env('GPP_FUSE_INPROJ_MIN_ROUNDS', FUSE_INPROJ_MIN_ROUNDS)),
        br1_lane=env('GPP_BR1_LANE', '1') != '0',           # measured +0.4 % on the f16x3 step (same box, alternating)
        fpn_lanes=fpn_lanes,
        p4_lane=1 if (fpn_lanes and env('GPP_P4_LANE', '1') != '0') else 0,
        head_lanes=head_lanes,
        decode_overlap=overlap,
        # GPP_CLS_LANE (default: on for B <= 2): at batch 1 a tower launch fields 0.9 - 1.9 rounds of workgroups of one wavefront per
        # SIMD: two independent chains in flight fill the other half of every SIMD (measured: profiles/r5/b1_latency.json, field
        # `plan_variants`); at batch 8 every launch fills the chip on its own (off)
        cls_lane=2 if (overlap and env('GPP_CLS_LANE', '1' if B <= 2 else '0') != '0') else 0,
        autotune=env('GPP_AUTOTUNE', '1') != '0',
        # GPP_SPARSE_HEADS (default 1; needs the decode overlap, whose candidate lists exist before the regression tower): the output
        # layers of the regression and dimension towers on the candidates' pixels only.  The value of the field is the largest share of
        # all pyramid pixels the gathered launches take (GPP_SPARSE_HEADS_MAX_SHARE; beyond it the dense launches run: the device
        # decides, per step); 0.0 = off.  An audit plan keeps the dense launches.
        sparse_heads=max(1e-9, float(env('GPP_SPARSE_HEADS_MAX_SHARE', SPARSE_HEADS_MAX_SHARE))) if sparse else 0.0,
        # GPP_SPARSE_TOWER (default 1; with sparse head outputs only): the regression tower's LAST layer on the 3 x 3 dilation of the
        # candidates' pixels -- the only rows its reader, the gathered output layer, takes.  The value is the largest share of all
        # pyramid pixels the gathered launch takes (GPP_SPARSE_TOWER_MAX_SHARE); GPP_SPARSE_TOWER_MIN_ROUNDS: the rounds of workgroups
        # the dense launch must exceed (0 in tests: small plans take the form too)
        sparse_tower=(max(1e-9, float(env('GPP_SPARSE_TOWER_MAX_SHARE', SPARSE_TOWER_MAX_SHARE)))
                      if (sparse and env('GPP_SPARSE_TOWER', '1') != '0') else 0.0),
        sparse_tower_rounds=float(env('GPP_SPARSE_TOWER_MIN_ROUNDS', SPARSE_TOWER_MIN_ROUNDS)),
        # GPP_SPARSE_TOWER_DEPTH (with the sparse tower only): how many layers of the regression tower run on the rows their
        # reader takes -- 1 the last layer alone, 2 layer 2 as well (the 5 x 5 dilation of the candidates' pixels), 3 layer 1 too (7 x 7),
        # 4 the regression slice of the fused first layer as well (9 x 9).
        # The lists of layers 2 and 1 are made from the logits on the caller's stream (gpp_detect_deep_lists);
        # GPP_SPARSE_TOWER_DEEP_MAX_SHARE: the largest share of rows their gathered launches take; GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS: the
        # rounds of workgroups their dense launch must exceed (its own variable: tests force the tower's to 0 at small shapes)
        sparse_deep=max(1e-9, float(env('GPP_SPARSE_TOWER_DEEP_MAX_SHARE', SPARSE_TOWER_DEEP_MAX_SHARE))),
        sparse_deep_rounds=float(env('GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS', SPARSE_TOWER_DEEP_MIN_ROUNDS)),
        sparse_depth=int(env('GPP_SPARSE_TOWER_DEPTH', SPARSE_TOWER_DEPTH)),
        # what of all this a cached tile choice depends on (models/tuning.py), the same at every batch: the variables as they are set
        tune_key='x3split={};fuse={}/{};plan={}{}'.format(x3_split, tail_widths, block_widths, model.plan_mode,
                                                          C.latency_split_config() if model.plan_mode == 'latency' else '') +
                 (';audit' if model.audit else '') + ('' if inproj else ';inproj=0'))      # (the default keeps its key)


# the fused projection block: its workgroups compute 8 x 14 output pixels, two share a compute unit
INPROJ_TILE = (8, 14)
FUSE_INPROJ_MIN_ROUNDS = '1'


def inproj_rounds(images, h, w):
    """ rounds of 2 x COMPUTE_UNITS workgroups the fused projection block of `images` images of h x w output pixels fields """
    th, tw = INPROJ_TILE
    return images * (-(-h // th)) * (-(-w // tw)) / (2.0 * COMPUTE_UNITS)


def block_form(opts, width, projection, split_input, halves, join, inproj=None):
    """ how one bottleneck runs: (launch, shortcut).
    launch: 'block' (branch2a + 2b + 2c + shortcut as one launch, gpp_bottleneck_block: pre-split input maps only), 'tail' (branch2a, then
    2b + 2c as one launch, gpp_bottleneck_tail) or 'convs' (three launches).
    inproj: (stride, images, h, w) of a projection block's batch part -- a rule of layer, map size and batch part, like the split rule: a
    stride-1 projection block of width 64 (res2a) whose launch fields MORE than opts.fuse_inproj_rounds rounds of workgroups runs as
    ('block', 'inproj'): one launch, gpp_bottleneck_block_proj, the shortcut computed inside it (float32 or pre-split input).
    shortcut: 'identity' (the block's input), 'side' (the projection on side lane 1, beside branch2a / 2b, joined by the launch that adds
    it) or 'inline' (the projection on the block's own lane: GPP_BR1_LANE=0, half-batch stages, and the first block behind a split stage,
    whose first launch joins the half-batch lanes). """
    if (projection and inproj is not None and opts.fuse_block_inproj and width == 64 and width in opts.fuse_block and inproj[0] == 1 and
            inproj_rounds(*inproj[1:]) > opts.fuse_inproj_rounds):
        return 'block', 'inproj'
    if width in opts.fuse_block and (not projection or opts.fuse_block_proj) and split_input:    # (res2a reads the pooled map: float32)
        launch = 'block'
    else:
        launch = 'tail' if width in opts.fuse_tail else 'convs'
    if not projection:
        return launch, 'identity'
    return launch, 'side' if opts.br1_lane and not halves and not join else 'inline'


def layer_split(plan_mode, shape, pixels):
    """ the split-K factor the rule of this plan mode gives a layer of shape (kh, kw, cin, cout) with `pixels` output pixels per image: the
    one place that chooses between the two rules (layers/conv.py).  A throughput plan's descriptors leave the factor to the library, whose
    rule default_split restates; the forms below need it before a descriptor exists """
    return (C.latency_split if plan_mode == 'latency' else C.default_split)(*shape, pixels)


# what head_forms decides: sparse = the plan has sparse head outputs at all (a SparseHeads); outputs = {output layer: 'dense' | 'pair' |
# 'lists_after'}; tower_both = pyramid_regression_3 takes both forms; deep_layers = how many tower layers in front of it do (0, 1, 2);
# tower0 = the regression slice of pyramid_towers_0 does too, as a launch pair behind pyramid_classification's lists
HeadForms = collections.namedtuple('HeadForms', 'sparse outputs tower_both deep_layers tower0')
HeadForms.__new__.__defaults__ = (False,)
TOWER0 = 'pyramid_towers_0'
TOWER0_SLICE = 512          # channels [0, 512) of the fused first layer's map are layer 0 of the regression tower (TOWER_SLICES)
HEAD_OUTPUTS = ('pyramid_classification', 'pyramid_regression_ops', 'pyramid_regression_dim')


def head_forms(opts, dtype, plan_mode, osf, audit, layers, deep_lists, levels, B, deferred=True):
    """ the form of every head layer that has more than one, named before anything is emitted (as block_form does for a bottleneck).
    layers: {name: (kh, kw, cin, cout)} of the three output layers and pyramid_regression_1 .. 3; deep_lists: the library has
    gpp_detect_deep_lists; levels: the (h, w) of the pyramid levels; B: the batch.  Every rule is one of layer, map sizes, batch and plan
    options, like the split rule -- never of a timing.

    An output layer is a 'pair' with opts.sparse_heads, regression and dimension tower: the decode reads these maps at candidate anchors
    only, so the layer runs in gathered-row form behind its guarded dense launch (PlanBuilder.out_layer).  A layer the split-K rule splits
    (small maps) keeps its dense launch alone: one gathered launch cannot reproduce that summation order.  pyramid_classification writes
    the logits the lists come from: always dense, 'lists_after' in a plan with deep layers (it makes their lists behind its launch).

    tower_both: pyramid_regression_3's reader pyramid_regression_ops is gathered in this plan, and the dense launch fields more than
    opts.sparse_tower_rounds rounds of 256 x 256 workgroups on the chip: below one round a gathered launch costs one workgroup life either way.

    deep_layers: the lists are made on the caller's stream right behind pyramid_classification, so that layer runs there, unsplit, with the
    candidate pass on its side lane (decode_overlap without cls_lane: no head_lanes), in a plan that is neither orientation-specific nor an
    audit; and the dense launch of a layer fields more than opts.sparse_deep_rounds rounds of workgroups

    tower0: both deep layers take the form, opts.sparse_depth >= 4, the library has gpp_conv2d_deferred_register
    (deferred), the plan is a throughput plan, `layers` names pyramid_towers_0, whose first TOWER0_SLICE columns are the regression tower's layer 0 -- a 256-column grid of
    layer 1's shape that fields more than opts.sparse_deep_rounds rounds -- and neither that slice nor the columns behind it are split """
    pixels = sum(h * w for h, w in levels)
    rows = sum((B * h * w + 255) // 256 for h, w in levels)

    def split(name):
        return layer_split(plan_mode, layers[name], pixels) > 1

    def fills(name, min_rounds):         # the layer's dense launch is a grid of 256 x 256 workgroups that fields more than min_rounds rounds
        cout = layers[name][3]
        return not cout % 256 and rows * (cout // 256) > min_rounds * COMPUTE_UNITS

    sparse = bool(opts.sparse_heads)
    tower_both = bool(sparse and opts.sparse_tower and opts.decode_overlap and opts.x3_level >= 1 and dtype in C.X3_TYPES and
                      not split('pyramid_regression_ops') and not split('pyramid_regression_3') and
                      fills('pyramid_regression_3', opts.sparse_tower_rounds))
    deep_layers = 0
    if (tower_both and opts.sparse_deep and opts.sparse_depth >= 2 and deep_lists and
            not (opts.cls_lane or opts.head_lanes or osf or audit) and
            not any(split(n) for n in ('pyramid_classification', 'pyramid_regression_1', 'pyramid_regression_2')) and
            not layers['pyramid_regression_1'][3] % 256 and fills('pyramid_regression_2', opts.sparse_deep_rounds)):
        deep_layers = min(2, opts.sparse_depth - 1)
    tower0 = False
    if deep_layers == 2 and opts.sparse_depth >= 4 and deferred and plan_mode != 'latency' and layers.get(TOWER0) is not None:
        kh, kw, cin, cout = layers[TOWER0]
        parts = {'slice': (kh, kw, cin, TOWER0_SLICE), 'rest': (kh, kw, cin, cout - TOWER0_SLICE)}
        tower0 = bool(cout > TOWER0_SLICE and layers['pyramid_regression_1'][2] == TOWER0_SLICE and
                      not any(layer_split(plan_mode, shape, pixels) > 1 for shape in parts.values()) and
                      rows * (TOWER0_SLICE // 256) > opts.sparse_deep_rounds * COMPUTE_UNITS)
    outputs = {name: 'dense' if not sparse or name == 'pyramid_classification' or split(name) else 'pair' for name in HEAD_OUTPUTS}
    if sparse and deep_layers:
        outputs['pyramid_classification'] = 'lists_after'
    return HeadForms(sparse, outputs, tower_both, deep_layers, tower0)


def part_of(fm, c0, nb):
    """ images [c0, c0 + nb) of a map """
    return C.FMap(fm.buf, nb, fm.H, fm.W, fm.C, off=fm.off + c0 * fm.bstride, bstride=fm.bstride, pitch=fm.pitch, split=fm.split, half=fm.half)


# RetinaNet3D(range_audit=True): the fused first layer of the three towers writes one 896-channel map whose slices the towers read
TOWER_SLICES = {('pyramid_towers_0', 0): 'pyramid_regression_0', ('pyramid_towers_0', 512): 'pyramid_classification_0',
                ('pyramid_towers_0', 768): 'pyramid_regression_dim_0'}
# the (hi, lo) IEEE-half pair is a fixed-point number with a quantum of 2^-24: a map whose LARGEST value is below
# 2^-9 keeps fewer than 16 significant bits of it, i.e. the whole map is stored at bf16x3 grade or worse
RANGE_AUDIT_THRESHOLD = 2.0 ** -9
X3_QUANTUM = 2.0 ** -24
# sparse head outputs: the share of listed rows up to which the gathered launches run (where their time crosses the dense launches')
SPARSE_HEADS_MAX_SHARE = '0.5'
# sparse regression tower: the share of rows in the DILATED lists up to which the gathered launch of the tower's last layer runs (DESIGN.md
# section 4.19: where its time crosses the dense launch's), and how many rounds of 256 x 256 workgroups on the chip's 256 compute units the
# dense launch must exceed for the layer to take the form at all (below one round either launch costs one workgroup life)
SPARSE_TOWER_MAX_SHARE = '0.75'
SPARSE_TOWER_MIN_ROUNDS = '1'
# ... and layers 2 and 1 of that tower on the 5 x 5 and 7 x 7 dilations: how many tower layers take both forms
# (1: the last one only), the share of rows up to which their gathered launches run (the last share measured below the dense launch for this
# kernel and shape, section 4.19's table), and the rounds their dense launch must exceed -- a variable of its own: tests pin what small
# plans do under GPP_SPARSE_TOWER_MIN_ROUNDS=0
SPARSE_TOWER_DEPTH = '4'
SPARSE_TOWER_DEEP_MAX_SHARE = '0.75'
SPARSE_TOWER_DEEP_MIN_ROUNDS = '1'
COMPUTE_UNITS = 256


def audit_report(maps, table, threshold=RANGE_AUDIT_THRESHOLD):
    """ the host side of the range audit: maps = Plan.audit_maps (name, consumers, channels, row = (first word, words)), table = the
    uint32 abs-max table of one run.  One record per map:
      name, consumers, channels; live = channels whose maximum is not zero; absmax = the map's largest |x| (NaN when a channel holds one);
      absmax_min_live / absmax_median_live over the live channels; small_channels = live channels whose maximum is below the threshold
      (INFORMATION only: every sane model has some); bits = floor(log2(absmax / 2^-24)) capped at 22: how many bits the map's largest
      value keeps in an IEEE-half pair; flagged = 0 < absmax < threshold -- the whole MAP sits in the fixed-point regime.  That is a
      sufficient condition for damage, not a necessary one: a few tiny channels with huge weights inside a map of ordinary size are
      reported (small_channels) and do not trigger.  A NaN maximum is the upper-range counter's business, not flagged here. """
    table = np.ascontiguousarray(table).view(np.uint32).reshape(-1)
    out = []
    for m in maps:
        first, n = m['row']
        bits = table[first:first + n]
        vals = bits.view(np.float32).astype(np.float64)
        live = vals[bits != 0]
        finite = live[~np.isnan(live)]
        absmax = float('nan') if len(finite) < len(live) else float(finite.max()) if len(finite) else 0.0
        rec = {k: m[k] for k in ('name', 'consumers', 'channels') if k in m}
        rec.update({'live': int(len(live)), 'absmax': absmax,
                    'absmax_min_live': float(finite.min()) if len(finite) else None,
                    'absmax_median_live': float(np.median(finite)) if len(finite) else None,
                    'small_channels': int((finite < threshold).sum()),
                    'bits': None if not absmax > 0 else int(min(22, max(0, np.floor(np.log2(absmax / X3_QUANTUM))))) if np.isfinite(absmax) else 22,
                    'flagged': bool(0 < absmax < threshold)})
        out.append(rec)
    return out


class SparseHeads(object):
    """ what the gathered head output layers of a plan share: the device lists gpp_detect_pixel_lists writes behind the candidate pass
    (bitmap, rows, counts, flag), the guarded dense descriptors (Plan.complete_heads) and the gathered ones (the tuner) """

    def __init__(self, torch, device, B, level_pixels, max_share, level_widths=None, tower_share=0.0):
        i32 = torch.int32
        self.B, self.level_pixels = B, [int(p) for p in level_pixels]
        self.level_widths = [int(w) for w in level_widths] if level_widths else []
        total = B * sum(self.level_pixels)
        self.max_rows = max(0, min(total, int(max_share * total)))
        self.bitmap = torch.zeros((sum((B * p + 31) // 32 for p in self.level_pixels),), dtype=i32, device=device)
        self.rows = torch.zeros((total,), dtype=i32, device=device)
        self.counts = torch.zeros((hip.GPP_MAX_GROUPS + 1,), dtype=i32, device=device)
        # 1: more rows than max_rows are listed -- the dense launches run and the gathered ones return at once; 0: the other way round.
        # 1 until a run's lists say otherwise, so that a single op run on its own (the per-layer tests) writes its whole map
        self.flag = torch.ones((1,), dtype=i32, device=device)
        self.dense, self.gathered = [], []
        self.lists_joined = False
        # the DILATED lists (tower_share > 0: the plan runs the regression tower's last layer on them, PlanBuilder.heads): the listed pixels
        # and their eight neighbours, what the gathered 3 x 3 output layer reads.  Same layout; tower_flag = flag | (more than tower_max_rows
        # rows).  tower = the descriptors of the layers that take both forms (Plan.complete_heads); range_scratch: where a completion's
        # dense re-run counts its range events (the run itself has counted the listed rows already)
        self.tower, self.tower_max_rows = [], 0
        self.tower_bitmap = self.tower_rows = self.tower_counts = self.tower_flag = self.range_scratch = None
        if tower_share > 0.0:
            self.tower_max_rows = max(0, min(total, int(tower_share * total)))
            self.tower_bitmap = torch.zeros_like(self.bitmap)
            self.tower_rows = torch.zeros_like(self.rows)
            self.tower_counts = torch.zeros_like(self.counts)
            self.tower_flag = torch.ones_like(self.flag)
            self.range_scratch = torch.zeros((1,), dtype=torch.int64, device=device)

        # the DEEP lists (add_deep): the rows of tower layers 2 and 1, written on the caller's stream behind the layer that writes the logits
        self.deep, self.deep_layers, self.deep_max_rows, self.deep_handle = [], 0, 0, 0
        self.deep_bitmaps = self.deep_rows = self.deep_counts = self.deep_flags = self.deep_stats = None
        # LAYER 0 (add_tower0): the regression slice of the towers' fused first layer on the radius-4 map of the same call.  Attributes of
        # their own, not members of the deep_* lists: tower0 = the slice's descriptor (both forms on tower0_rows / tower0_counts /
        # tower0_flag), which the library keeps a copy of (tower0_handle) and enqueues behind the lists of tower0_carrier, the descriptor
        # of the layer that writes the logits (gpp_conv_desc.conv_after)
        self.tower0 = self.tower0_carrier = None
        self.tower0_handle = 0
        self.tower0_bitmap = self.tower0_rows = self.tower0_counts = self.tower0_flag = self.tower0_stats = None

    def add_tower0(self, torch):
        """ the buffers of layer 0's lists (gpp_deep_list_desc.radius4 / rows0 / counts0 / flag0 / stats0); the flag starts at 1 """
        self.tower0_bitmap = torch.zeros_like(self.bitmap)
        self.tower0_rows = torch.zeros_like(self.rows)
        self.tower0_counts = torch.zeros_like(self.counts)
        self.tower0_flag = torch.ones_like(self.flag)
        self.tower0_stats = torch.zeros_like(self.flag)

    def tower0_tensors(self):
        if self.tower0_rows is None:
            return []
        return [self.tower0_bitmap, self.tower0_rows, self.tower0_counts, self.tower0_flag, self.tower0_stats]

    def register_tower0(self, desc=None, carrier=None):
        """ hands the slice's descriptor to the library and its handle to the carrier (gpp_conv_desc.conv_after); without arguments: again,
        after the tuner has written the tiles into the descriptor -- the library holds a copy """
        self.tower0, self.tower0_carrier = desc or self.tower0, carrier or self.tower0_carrier
        lib, handle = hip.lib(), ctypes.c_int32(0)
        if self.tower0_handle:
            hip.check(lib.gpp_conv2d_deferred_release(self.tower0_handle), 'gpp_conv2d_deferred_release')
            self.tower0_handle = 0
        hip.check(lib.gpp_conv2d_deferred_register(ctypes.byref(self.tower0), ctypes.byref(handle)), 'gpp_conv2d_deferred_register')
        self.tower0_handle = self.tower0_carrier.conv_after = int(handle.value)

    def add_deep(self, torch, layers, deep_share):
        """ the buffers of gpp_detect_deep_lists for `layers` (1: layer 2 only, 2: layers 2 and 1) tower layers in front of the last one: the
        marks and the three dilation bitmaps, a row list, a count vector and a flag per layer (index 0: layer 2 on the radius-2 map, index 1:
        layer 1 on the radius-3 map), and the call's statistics.  The flags start at 1, like every flag here.  deep = [descriptor of layer 1,
        descriptor of layer 2], in layer order (Plan.complete_heads) """
        total = self.B * sum(self.level_pixels)
        self.deep_layers = int(layers)
        self.deep_max_rows = max(0, min(total, int(deep_share * total)))
        self.deep_bitmaps = [torch.zeros_like(self.bitmap) for _ in range(4)]
        self.deep_rows = [torch.zeros_like(self.rows) for _ in range(self.deep_layers)]
        self.deep_counts = [torch.zeros_like(self.counts) for _ in range(self.deep_layers)]
        self.deep_flags = [torch.ones_like(self.flag) for _ in range(self.deep_layers)]
        self.deep_stats = torch.zeros((4,), dtype=torch.int32, device=self.rows.device)

    def deep_tensors(self):
        if self.deep_rows is None:
            return []
        return self.deep_bitmaps + self.deep_rows + self.deep_counts + self.deep_flags + [self.deep_stats]

    def deep_desc(self, cls_logits, n_anchors, num_base_anchors, score_thr):
        """ the gpp_deep_list_desc of these buffers """
        d = hip.DeepListDesc()
        d.cls_logits = cls_logits.data_ptr()
        d.marks, d.radius1, d.radius2, d.radius3 = [t.data_ptr() for t in self.deep_bitmaps]
        d.rows2, d.counts2, d.flag2 = self.deep_rows[0].data_ptr(), self.deep_counts[0].data_ptr(), self.deep_flags[0].data_ptr()
        if self.deep_layers > 1:
            d.rows1, d.counts1, d.flag1 = self.deep_rows[1].data_ptr(), self.deep_counts[1].data_ptr(), self.deep_flags[1].data_ptr()
        d.stats = self.deep_stats.data_ptr()
        if self.tower0_rows is not None:
            d.radius4, d.rows0, d.counts0 = self.tower0_bitmap.data_ptr(), self.tower0_rows.data_ptr(), self.tower0_counts.data_ptr()
            d.flag0, d.stats0 = self.tower0_flag.data_ptr(), self.tower0_stats.data_ptr()
        d.n_anchors, d.B, d.num_base_anchors, d.n_levels = n_anchors, self.B, num_base_anchors, len(self.level_pixels)
        d.max_rows, d.tower_max_rows, d.deep_max_rows, d.score_thr = self.max_rows, self.tower_max_rows, self.deep_max_rows, score_thr
        d.level_pixels = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*self.level_pixels)
        d.level_width = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*self.level_widths)
        return d

    def register_deep(self, desc):
        """ the library keeps a copy of the descriptor; gpp_conv_desc.lists_after names it by the handle returned here """
        handle = ctypes.c_int32(0)
        hip.check(hip.lib().gpp_detect_deep_lists_register(ctypes.byref(desc), ctypes.byref(handle)), 'gpp_detect_deep_lists_register')
        self.deep_handle = int(handle.value)
        return self.deep_handle

    def __del__(self):
        if getattr(self, 'deep_handle', 0):
            try:
                hip.lib().gpp_detect_deep_lists_release(self.deep_handle)
            except Exception:          # (interpreter shutdown)
                pass
            self.deep_handle = 0
        if getattr(self, 'tower0_handle', 0):
            try:
                hip.lib().gpp_conv2d_deferred_release(self.tower0_handle)
            except Exception:
                pass
            self.tower0_handle = 0

    def tensors(self):
        own = [self.bitmap, self.rows, self.counts, self.flag]
        return own + ([self.tower_bitmap, self.tower_rows, self.tower_counts, self.tower_flag] if self.tower_rows is not None else [])

    def put_every_nth(self, torch, n=8, tower=False):
        """ a synthetic list for the tuner: every n-th pixel of every level (tower: into the dilated lists) """
        rows, cnt = (self.tower_rows, self.tower_counts) if tower else (self.rows, self.counts)
        begin, counts = 0, []
        for p in self.level_pixels:
            idx = torch.arange(0, self.B * p, n, dtype=torch.int32, device=rows.device)
            rows[begin:begin + idx.numel()] = idx
            counts.append(int(idx.numel()))
            begin += self.B * p
        counts += [0] * (hip.GPP_MAX_GROUPS - len(counts)) + [sum(counts)]
        cnt.copy_(torch.as_tensor(counts, dtype=torch.int32))

    def reset(self, torch):
        """ nothing listed, the dense launches run: the state before the first run """
        self.counts.zero_()
        self.flag.fill_(1)
        if self.tower_rows is not None:
            self.tower_counts.zero_()
            self.tower_flag.fill_(1)
        self.reset_deep()

    def reset_deep(self):
        """ the deep flags at 1, ordered on the current stream: what an op run on its own leaves behind it (it writes its whole map) """
        for flag in list(self.deep_flags or ()) + ([self.tower0_flag] if self.tower0_flag is not None else []):
            flag.fill_(1)


class Plan(object):
    """ Everything one (batch, H, W, N planes) configuration needs: buffers, descriptors, op array. """

    def __init__(self):
        self.keep = []          # ctypes descriptors and torch buffers kept alive
        self.io = {}            # conv op name -> (input FMaps, output FMaps, residual FMaps or None); half-batch plans: the LAST part
        self.io_parts = {}      # conv op name -> [(inputs, outputs, residuals) of every launch under that name] (half-batch plans: two)
        self.tuning_parts = {}  # conv op name -> [(tile, us) of every launch under that name]
        self.ops = []           # (kind, tag, desc, name, flops)
        self.oracle_names = {}  # fused ops: reference layer name of each output map (per-layer parity tests)
        self.lanes = []         # per op: side-stream lane << 8 | join flag (include/gpp.h GPP_OP_LANE / GPP_OP_JOIN)
        self.access = []        # per op: (byte intervals read, byte intervals written): check_stream_ordering
        self.atomic = []        # per op: byte intervals it only updates with order-free atomics (the abs-max rows of an audit plan)
        self.wrote = []         # per op: the FMaps among its writes; per op: its io record (audit plans: who produces, who reads a map)
        self.op_io = []
        self.audit_table = None     # RetinaNet3D(range_audit=True): see PlanBuilder.audit
        self.audit_maps = []
        self.audit_unobserved = []
        self.inner = {}         # id(descriptor) -> the gpp_conv_desc records a fused or pre-activation launch points to
        self.open_lanes = set()  # side lanes forked and not joined by the ops recorded so far
        self.conv_descs = []    # (gpp_conv_desc, stream lane): the split-K workspace of each lane is bound once every op is known
        self.ws_need = {}       # stream lane -> the largest split-K workspace one of its conv descriptors needs
        self.array = None
        self.flops = 0.0
        self.ragged = False     # plan_for(..., ragged=True): the plan of a height class; heights = its int32 device table, heights_host = what it holds
        self.heights = None
        self.sparse = None      # SparseHeads: the head output layers run on the candidates' pixels only (PlanBuilder.heads)
        self.heads_stale = False    # a run has left rows of regression / regression_dim unwritten: the next read of either completes them

    # The two regression head tensors.  With sparse head outputs a run writes them at the pixels the decode reads and nowhere else; whoever
    # reads a whole tensor (tests, bench.py --full, the CPU replay of the decode) gets it whole: the first read after such a run enqueues the
    # two dense launches -- the descriptors a dense plan runs, on the current stream -- and the listed rows keep their bytes (a gathered row
    # IS the dense row).  In a plan whose regression tower ends in a layer of both forms (SparseHeads.tower) that layer is run dense first:
    # the output layer's dense launch reads every row of it.  predict_on_batch, run_plan and fetch never come here.
    @property
    def regression(self):
        self.complete_heads()
        return self._regression

    @regression.setter
    def regression(self, tensor):
        self._regression = tensor

    @property
    def regression_dim(self):
        self.complete_heads()
        return self._regression_dim

    @regression_dim.setter
    def regression_dim(self, tensor):
        self._regression_dim = tensor

    def complete_heads(self):
        if self.sparse is None or not self.heads_stale:
            return
        self.heads_stale = False
        sp = self.sparse
        # layer 0's regression slice (in front of layer 1, inside its call), deep layers 1, 2 in layer order, then the tower's last layer, then the output layers: each dense reader reads every row of the layer
        # in front.  Each is the dense launch as it stands in the plan, without its lists or its guard; a layer of both forms counts its range
        # events into a scratch slot: the run has counted those of the rows it wrote
        for descs, lists, tile, scratch, what in (
                (sp.deep, ('deep_rows', 'deep_counts', 'deep_flag'), 'deep_tile', True, 'deep tower layer completed'),
                (sp.tower, ('tower_rows', 'tower_counts', 'tower_flag'), 'tower_tile', True, 'tower layer completed'),
                (sp.dense, ('guard',), 'guard_value', False, 'head tensors completed')):
            for desc in descs:
                d = type(desc).from_buffer_copy(desc)
                for field in lists:
                    setattr(d, field, None)
                setattr(d, tile, 0)
                if scratch and d.range_counter:
                    d.range_counter = sp.range_scratch.data_ptr()
                if sp.tower0 is not None and desc is sp.deep[0]:
                    # layer 1 reads every row of layer 0's regression slice, which the run wrote on the radius-4 rows: the library runs the
                    # copy it holds dense in front of this launch, into the same counter (gpp_conv_desc.conv_before)
                    d.conv_before = sp.tower0_handle
                hip.check(hip.lib().gpp_conv2d_igemm(ctypes.byref(d), hip.stream_ptr()), 'gpp_conv2d_igemm ({})'.format(what))

    def emit(self, kind, desc, name, reads=(), writes=(), tag=0, flops=0.0, lane=0, join=False, sync=False, io=None, inner=(), atomic=()):
        """ record one launch.  reads / writes: the FMaps and tensors it reads and writes (check_stream_ordering); io: its
        (inputs, outputs, residuals) FMaps for the per-layer tests; inner: the conv descriptors its descriptor points to; atomic: what
        it only updates with atomics whose result does not depend on their order (two such launches may run side by side) """
        self.keep += list(inner) + [desc]
        if inner:
            self.inner[id(desc)] = tuple(inner)
        self.ops.append((kind, tag, desc, name, flops))
        self.lanes.append((int(lane) << 8) | (OP_JOIN if join else 0) | (OP_SYNC if sync else 0))
        self.access.append((self.spans(reads), self.spans(writes)))
        self.atomic.append(self.spans(atomic))
        self.wrote.append([x for x in writes if isinstance(x, C.FMap)])
        self.op_io.append(io)
        self.flops += flops
        if lane:
            self.open_lanes.add(lane)
        elif join:
            self.open_lanes.clear()
        if io is not None:
            self.io[name] = io
            self.io_parts.setdefault(name, []).append(io)

    # ---- who reads and writes what: the byte intervals (one per image) every launch touches.  check_stream_ordering() replays
    # gpp_plan_run's fork / join rules over them: the plan builder places launches on side streams by hand, and a missing join is
    # a race that shows up once in a while, at full size only (round 4 found one between a split and an unsplit stage)
    @staticmethod
    def span(fm):
        """ byte intervals of an FMap, one per image """
        e = fm.buf.element_size()
        base = fm.buf.data_ptr() + fm.off * e
        size = ((fm.H * fm.W - 1) * fm.pitch + fm.C) * e
        return [(base + b * fm.bstride * e, base + b * fm.bstride * e + size) for b in range(fm.B)]

    @staticmethod
    def span_of(tensor):
        return [(tensor.data_ptr(), tensor.data_ptr() + tensor.numel() * tensor.element_size())]

    @staticmethod
    def spans(items):
        """ byte intervals of a list of FMaps and tensors """
        return [iv for x in items for iv in (Plan.span(x) if isinstance(x, C.FMap) else Plan.span_of(x))]

    def insert_behind(self, extra):
        """ extra: {position: [(kind, desc, name, FMaps read, tensors updated atomically)]}: records these launches directly behind the
        op at that position, on its lane (no join, no fork of their own) -- the audit launches, placed once every reader of every map is known """
        old = (self.ops, self.lanes, self.access, self.atomic, self.wrote, self.op_io)
        self.ops, self.lanes, self.access, self.atomic, self.wrote, self.op_io = [], [], [], [], [], []
        for pos, row in enumerate(zip(*old)):
            for dst, item in zip((self.ops, self.lanes, self.access, self.atomic, self.wrote, self.op_io), row):
                dst.append(item)
            for kind, desc, name, reads, atomic in extra.get(pos, ()):
                self.keep.append(desc)
                self.ops.append((kind, 0, desc, name, 0.0))
                self.lanes.append(row[1] & 0xff00)
                self.access.append((self.spans(reads), []))
                self.atomic.append(self.spans(atomic))
                self.wrote.append([])
                self.op_io.append(None)

    def check_stream_ordering(self):
        """ every pair of launches on DIFFERENT streams that touch overlapping bytes (at least one of them writing) must be ordered by a
        fork or a join, as gpp_plan_run (csrc/plan.cpp) places them: a side-lane launch forks from the caller's stream when its lane is
        not open (or carries SYNC); a JOIN launch on the caller's stream (and the end of the plan) closes every open lane.
        Returns the list of violations [(earlier op, later op)], empty when the plan is race-free by construction. """
        def overlap(a, b):
            return any(x0 < y1 and y0 < x1 for x0, x1 in a for y0, y1 in b)
        bad, seen = [], []                    # seen: (position, lane, name, reads, writes, atomic updates)
        active = {}
        forks, joins = {}, []                 # lane -> positions of its forks; positions of joins
        for pos, (kind, _, desc, name, _) in enumerate(self.ops):
            flags = self.lanes[pos]
            lane, join, sync = (flags >> 8) & 0xff, bool(flags & OP_JOIN), bool(flags & OP_SYNC)
            if lane > 0:
                if not active.get(lane) or sync:
                    forks.setdefault(lane, []).append(pos)
                    active[lane] = True
            elif join:
                joins.append(pos)
                active = {}
            reads, writes = self.access[pos]
            atomic = self.atomic[pos]
            for p0, l0, n0, r0, w0, a0 in seen:
                # (two order-free atomic updates of the same bytes do not conflict; an atomic update and a plain access do)
                if l0 == lane or not (overlap(w0, reads) or overlap(w0, writes) or overlap(r0, writes) or overlap(a0, reads) or
                                      overlap(a0, writes) or overlap(w0, atomic) or overlap(r0, atomic)):
                    continue
                j = [q for q in joins if p0 < q <= pos]                      # a join after the earlier launch, not after this one
                if l0 == 0:
                    ok = any(p0 < f <= pos for f in forks.get(lane, []))     # this lane forked after the main-stream launch
                elif lane == 0:
                    ok = bool(j)
                else:
                    ok = bool(j) and any(min(j) <= f <= pos for f in forks.get(lane, []))
                if not ok:
                    bad.append((n0, name))
            seen.append((pos, lane, name, reads, writes, atomic))
        return bad

    @staticmethod
    def stage_of(kind, name):
        """ include/gpp.h GPP_OP_STAGE: 1 stem, 2 backbone, 3 FPN, 4 heads, 5 decode, 6 polling, 8 pose, 9 audit, 10 cuboid NMS (roctx ranges under GPP_ROCTX=1) """
        if kind in (OP_STEM, OP_MAXPOOL, OP_STEM_POOL, OP_MAXPOOL_PAD, OP_MOBILENET_STEM, OP_STEM_RAGGED, OP_STEM_POOL_RAGGED, OP_MAXPOOL_RAGGED):
            return 1
        if kind in DETECT_OPS:
            return 5
        if kind == OP_POLL:
            return 6
        if kind == OP_POSE:
            return 8
        if kind == OP_CUBOID_NMS:
            return 10
        if kind in (OP_ABSMAX, OP_ABSMAX_CLEAR):
            return 9
        if name.startswith('res') or kind in (OP_CONV_PREACT, OP_AVGPOOL, OP_MOBILENET_BLOCK) or name.startswith(('conv2_', 'conv3_', 'conv4_', 'conv5_')):
            return 2
        if name.startswith('pyramid_'):
            return 4
        return 3                                  # C5_reduced ... P3, P6, C6_relu, P7

    def finalize(self):
        arr = (PlanOp * len(self.ops))()
        for i, (kind, tag, desc, name, _) in enumerate(self.ops):
            arr[i].kind, arr[i].tag, arr[i].desc = kind | self.lanes[i] | (self.stage_of(kind, name) << 20), tag, ctypes.addressof(desc)
        self.array = arr
