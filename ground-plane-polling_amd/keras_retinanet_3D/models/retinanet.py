"""
RetinaNet-3D inference model on MI355X: the object `models.load_model` returns.

It plays the role of the keras.models.Model that the reference builds in
/root/reference/keras_retinanet_3D/models/retinanet.py:359-422 (`retinanet_bbox`):
    backbone (keras_resnet, models/resnet.py:88-102) -> C3, C4, C5
    __create_pyramid_features :170-205                -> P3..P7 (512 channels)
    regression / regression_dim / classification heads :24-167, applied per level, concatenated :257-281
    Anchors + RegressBoxes + RegressDims :284-311, :411-412 ; FilterDetections :415 ; FitRoadPlanes :416
with the same `predict_on_batch([images, P_inv, planes])` -> 8 arrays contract
(bin/run_network.py:105-110; output order retinanet.py:418-419).

Nothing is traced or compiled at run time: for a given (batch, H, W) the model lays out its
activations in HBM once and records a *plan* -- a flat array of C-ABI descriptors (include/gpp.h) --
that one `gpp_plan_run` call enqueues on the current HIP stream.  All arithmetic happens in the
hand-written kernels of ../csrc; PyTorch only owns the device buffers.  The model here owns the weights and the plans per shape and runs
them; one PlanBuilder (models/builder.py) records each plan, models/tuning.py chooses its tiles.

HBM layout
  * activations NHWC, 16-bit (bf16 default, f16) or float32 (dtype='f32': the reference's own arithmetic type --
    float32 operands on v_mfma_f32_16x16x4_f32, float32 stem, no fused bottleneck tails; dtype='bf16x3': the same float32
    storage with every float32 product computed as three bf16 matrix products, ~2^-16 relative), one dense buffer per live tensor
  * the five pyramid levels of every FPN / head tensor are stored back to back per image,
    (B, 11438, C) for a 402x1333 input, so that one grouped launch covers all levels and the head
    outputs come out directly in the reference's concatenated (B, A, k) order
  * head outputs (classification logits, fused 144-channel regression, dimensions) float32
  * weights [C_out][KH*KW*C_in] in the storage type with the frozen BatchNormalization folded in, biases float32
Every bit of a result is a function of (image, weights, dtype) alone: block tiles are tuned by timing but never change
a result, and split-K follows a rule of the layer alone (gpp_conv2d_split_rule) -- not of the batch size or the rank.
"""

import ctypes
import os

import numpy as np

from ..backend import hip
from ..layers import conv as C
from ..layers import mobilenet as M
from ..utils import cuboid_nms as cuboid_nms_utils
from ..utils import track as track_utils
from . import tuning
from . import weights as W
from .builder import PlanBuilder
# what a plan is (models/plan.py), under the names this module has always had: tests and tools spell them retinanet.StemDesc, retinanet.OP_CONV ...
from .plan import (BlockDesc, BlockProjDesc, FUSE_INPROJ_MIN_ROUNDS, CandidatePixelsDesc, DensePoolDesc, DetectDesc, PlanOp, PollDesc, PoolDesc, PoseDesc, CuboidNmsDesc,  # noqa: F401
                   PreactDesc, RaggedPoolDesc, RaggedStemDesc, ReluDesc, StemDesc, TailDesc,
                   OP_STEM, OP_MAXPOOL, OP_CONV, OP_RELU, OP_DETECT, OP_POLL, OP_TAIL, OP_BLOCK,
                   OP_DETECT_CANDIDATES, OP_DETECT_SELECT, OP_DETECT_EMIT, OP_DETECT_OSF, OP_STEM_POOL,
                   OP_MAXPOOL_PAD, OP_AVGPOOL, OP_CONV_PREACT, OP_MOBILENET_STEM, OP_MOBILENET_BLOCK, OP_POSE, OP_CUBOID_NMS,
                   OP_ABSMAX, OP_ABSMAX_CLEAR, OP_STEM_RAGGED, OP_STEM_POOL_RAGGED, OP_MAXPOOL_RAGGED,
                   OP_DETECT_CANDIDATE_PIXELS, DETECT_OPS, OP_JOIN, OP_SYNC,
                   PlanOptions, block_form, part_of, plan_options, TOWER_SLICES, TOWER0, RANGE_AUDIT_THRESHOLD, X3_QUANTUM,
                   SPARSE_HEADS_MAX_SHARE, SPARSE_TOWER_MAX_SHARE, SPARSE_TOWER_MIN_ROUNDS, SPARSE_TOWER_DEPTH,
                   SPARSE_TOWER_DEEP_MAX_SHARE, SPARSE_TOWER_DEEP_MIN_ROUNDS, COMPUTE_UNITS, audit_report, SparseHeads, Plan)


class RetinaNet3D(object):
    """ Inference model: ResNet-50/101/152, DenseNet-121/169/201 or MobileNet (v1) + FPN + heads + decode + ground-plane polling. """

    def __init__(self, weights, backbone_name='resnet50', dtype='f16x3', nms=True, class_specific_filter=True,
                 orientation_specific_filter=False, name='retinanet-bbox', on_range_event=None, plan=None, pose=False, range_audit=False,
                 cuboid_nms=None, track=None):
        import torch
        # range_audit=True (dtype='f16x3' only): every plan also measures the largest |x| of every channel of every map an x3 convolution
        # reads (gpp_channel_absmax, _audit), and a synchronous call whose run left a whole map below RANGE_AUDIT_THRESHOLD reacts as
        # on_range_event says.  A model attribute like `pose`: without it every plan is what it was, launch for launch
        self.audit = bool(range_audit)
        if self.audit and dtype != 'f16x3':
            raise ValueError("range_audit=True watches the lower range of dtype='f16x3', got dtype={!r}: the IEEE-half pair is a fixed-point "
                             "number with a quantum of 2^-24 below 2^-14; bf16 halves keep float32's exponent and have no such regime, "
                             "and the other types store no split halves".format(dtype))
        self.small_magnitude_events = 0      # flagged (call, map) pairs
        self.last_range_audit = None         # the report of the last synchronous call of an audit model
        self._last_plan = None
        # pose=True: every plan ends with the pose stage (gpp_pose_f32 on the polling outputs) and predict_poses_on_batch /
        # predict_poses_on_frames fetch its rows; a model attribute, not a plan switch: without it every plan is what it was
        self.pose = bool(pose)
        # cuboid_nms=(metric, threshold), metric 'bev' or '3d' (pose=True only): every plan ends with ONE more op behind the pose stage,
        # gpp_cuboid_nms_f64 in place on the pose rows -- a greedy NMS of the cuboids themselves; every reader
        # of the rows sees the suppressed set, cuboid_suppressors() says which row removed which.  A model attribute like `pose`; there
        # is no default threshold
        self.cuboid_nms = cuboid_nms_utils.check_option(cuboid_nms)
        if self.cuboid_nms is not None and not self.pose:
            raise ValueError('cuboid_nms={!r} suppresses pose rows: it needs pose=True'.format(cuboid_nms))
        # track=(metric, threshold) or a dict (utils/track.check_option; pose=True only): predict_tracks_on_frames / _on_batch follow the plan
        # with ONE more launch, gpp_track_f64 -- not a plan op: every plan and every other method is what it was.
        # The images of a call are consecutive frames of the model's one sequence; the state lives in HBM between the calls.  With
        # 'ego': True the two methods take the frames' ego records and the launch is gpp_track_ego_f64 (section 4.33)
        self.track = track_utils.check_option(track)
        if self.track is not None and not self.pose:
            raise ValueError('track={!r} associates pose rows: it needs pose=True'.format(track))
        self._track_state = None             # (current, next): two (1, gpp_track_state) buffers, swapped after every answered call
        self._track_cov = None               # 'filter': 'kalman' (section 4.34): (current, next), two (1, gpp_track_cov) buffers, swapped with them
        self._answered = None                # (model, plan) that answered the last call of the pose family
        # 'throughput' | 'latency' (models.load_model): which layers split their K loop (layers/conv.latency_split)
        self.plan_mode = plan or os.environ.get('GPP_PLAN', 'throughput')
        if self.plan_mode not in ('throughput', 'latency'):
            raise ValueError("plan must be 'throughput' or 'latency', got {!r}".format(self.plan_mode))
        # dtype='f16x3' only -- what happens when an activation of a call left the IEEE-half range (a finite value beyond +-65504 is
        # clamped when it is split: a plausible wrong answer; the epilogues count such stores, gpp_x3_range_events):
        #   'f32' (default)  the call is run again at dtype='f32' (a float32 twin of the model, built at the first event) and THAT result
        #                    is returned: the drop-in returns what the reference's floatx graph returns, slower for that call
        #   'raise'          GppError
        #   'ignore'         rounds 3-4: the counter is only there to be read (model.x3_range_events())
        # The counter is read with the results a synchronous call fetches anyway (fetch(), FramePipeline): no extra synchronisation.
        self.on_range_event = on_range_event or os.environ.get('GPP_ON_RANGE_EVENT', 'f32')
        if self.on_range_event not in ('f32', 'raise', 'ignore'):
            raise ValueError("on_range_event must be 'f32', 'raise' or 'ignore', got {!r}".format(self.on_range_event))
        self.range_fallbacks = 0         # calls whose result was replaced (or refused) because of a range event
        self._twin = None
        self._weights = weights if (dtype == 'f16x3' and self.on_range_event == 'f32') else None
        self.class_specific_filter = class_specific_filter
        self.osf = bool(orientation_specific_filter)     # per-orientation NMS (filter_detections.py:84-98), gpp_detect_osf_f32
        self.nms = bool(nms)
        self.name = name
        self.mobilenet = W.is_mobilenet(backbone_name)           # 'mobilenet224_1.0': the name carries the width multiplier
        self.backbone_name = backbone_name if self.mobilenet else backbone_name.split('_')[0]
        self.densenet = W.is_densenet(self.backbone_name)
        if self.backbone_name not in W.BLOCKS and not self.densenet and not self.mobilenet:
            raise ValueError('Backbone (\'{}\') not in allowed backbones ({}).'.format(
                backbone_name, sorted(W.BLOCKS) + sorted(W.DENSENET_BLOCKS) + ['{}_<{}>'.format(r, '|'.join(str(a) for a in W.MOBILENET_ALPHAS))
                                                                              for r in W.MOBILENET_ROWS]))
        if dtype not in ('bf16', 'f16', 'f32', 'bf16x3', 'f16x3'):
            raise ValueError("dtype must be 'bf16', 'f16', 'f32', 'bf16x3' or 'f16x3', got {!r}".format(dtype))
        if self.densenet and dtype not in ('f32', 'f16x3', 'bf16x3'):
            # the concatenation buffers and the pre-activation 1x1 conv (gpp_conv2d_preact) exist for float32 storage only
            raise ValueError("a DenseNet backbone runs with dtype 'f32', 'f16x3' or 'bf16x3', got {!r}".format(dtype))
        if self.mobilenet and dtype not in ('f32', 'f16x3', 'bf16x3'):
            # the fused depthwise-separable block (gpp_mobilenet_block) and the stem exist for float32 storage only
            raise ValueError("a MobileNet backbone runs with dtype 'f32', 'f16x3' or 'bf16x3', got {!r}".format(dtype))
        self.dtype = dtype
        self.esz = C.elem_size(dtype)
        self.tdtype = C.torch_dtype(dtype)
        self.device = hip.require_device()
        hip.lib()
        self.torch = torch
        self._plans = {}
        self._anchors = {}
        self._taps, self._ragged_taps = {}, {}      # resize tap tables on the device, per frame size (stage_frames / _stage_ragged_frames)
        self.stem_x3 = False         # conv1 on the matrix pipe, input and weights split into two IEEE halves (_upload)
        self._tune = tuning.TuneCache.for_model(self)        # (layer, B, H, W) -> (tile, us): what _autotune has chosen or found in GPP_TUNE_CACHE
        self._tune.load(os.environ.get('GPP_TUNE_CACHE'))
        self._upload(weights)
        self.tag_names = []          # filled by the plan builder: names of event-tagged ops

    # ------------------------------------------------------------------ weights
    def _upload(self, weights):
        torch, dev = self.torch, self.device
        W.validate_weights(weights, self.backbone_name)
        self.conv_w = {}
        self.conv_scale = {}

        def put(name, kernel, bias):
            self.conv_w[name] = (C.pack_weight(kernel, self.dtype, dev), torch.as_tensor(bias).to(dev).contiguous(),
                                 kernel.shape)
            if self.dtype == 'f16x3':        # the inverse of the per-channel power of two the packed weights carry (layers/conv.py)
                self.conv_scale[name] = C.out_scale_of(kernel, dev)

        if self.densenet:
            self._upload_densenet(weights, put)
        if self.mobilenet:
            self._upload_mobilenet(weights)
        for conv, bn, kh, kw, cin, cout, _ in (() if self.densenet or self.mobilenet else W.backbone_layers(self.backbone_name)):
            k, b = W.folded_conv(weights, conv, bn)
            if k.shape != (kh, kw, cin, cout):
                raise ValueError('weight {} has shape {}, expected {}'.format(conv, k.shape, (kh, kw, cin, cout)))
            if conv == 'conv1':
                if self.dtype in C.X3_TYPES and os.environ.get('GPP_X3_STEM', 'mfma') != 'valu':
                    # the x3 types: conv1 on the matrix pipe, input and weights split into two IEEE halves (csrc/stem.hip)
                    self.stem_w = hip.pack_stem_weights_x3(k.reshape(147, 64), dev)
                    self.stem_x3 = True
                elif self.esz == 4:          # float32 stem on the vector ALUs: the folded kernel as it is, [147][64]
                    self.stem_w = torch.as_tensor(np.ascontiguousarray(k.reshape(147, 64), dtype=np.float32)).to(dev).contiguous()
                else:
                    self.stem_w = hip.pack_stem_weights(k.reshape(147, 64), dev)
                self.stem_b = torch.as_tensor(b).to(dev).contiguous()
            else:
                put(conv, k, b)
        for name, k_, cin, cout, _ in W.fpn_layers(self.backbone_name):
            k, b = W.folded_conv(weights, name)
            put(name, k, b)
        for name, cin, cout, kind in W.head_layers():
            if name.startswith('pyramid_regression_op'):
                continue
            k, b = W.folded_conv(weights, name)
            put(name, k, b)
        k, b = W.fused_regression_outputs(weights)
        put('pyramid_regression_ops', k, b)
        k, b = W.fused_tower_inputs(weights)
        put('pyramid_towers_0', k, b)

    def _upload_densenet(self, weights, put):
        """ DenseNet: conv1/conv with conv1/bn folded (the stem kernels), every _1_conv with its _1_bn folded (+ ReLU epilogue), _2_conv and
        the transition convs as they are (no bias), and the BatchNormalization in front of every 1x1 conv as a (scale, shift) pair for the
        prologue of gpp_conv2d_preact: it belongs to the consumer of a concatenation and cannot be folded into any producer """
        torch, dev, eps = self.torch, self.device, W.DENSENET_BN_EPSILON
        self.preact = {}
        k, b = W.folded_conv(weights, 'conv1/conv', 'conv1/bn', eps=eps)
        if self.dtype in C.X3_TYPES and os.environ.get('GPP_X3_STEM', 'mfma') != 'valu':
            self.stem_w = hip.pack_stem_weights_x3(k.reshape(147, 64), dev)
            self.stem_x3 = True
        else:
            self.stem_w = torch.as_tensor(np.ascontiguousarray(k.reshape(147, 64), dtype=np.float32)).to(dev).contiguous()
        self.stem_b = torch.as_tensor(b).to(dev).contiguous()
        pending = None
        for kind, name, shape in W.densenet_layers(self.backbone_name):
            if kind == 'bn':
                if name.endswith('_0_bn') or (name.startswith('pool') and name.endswith('_bn')):
                    pending = name
                continue
            if name == 'conv1/conv':
                continue
            if name.endswith('_1_conv'):
                k, b = W.folded_conv(weights, name, name[:-len('_1_conv')] + '_1_bn', eps=eps)
            else:
                k, b = np.asarray(weights[name + '/kernel'], dtype=np.float32), np.zeros((shape[3],), np.float32)
            put(name, k, b)
            if shape[0] == 1:                   # the 1x1 convs: _1_conv and the transitions, behind the BN + ReLU just seen
                s, t = W.bn_affine(weights, pending, eps)
                self.preact[name] = (torch.as_tensor(s).to(dev).contiguous(), torch.as_tensor(t).to(dev).contiguous())

    def _upload_mobilenet(self, weights):
        """ MobileNet: conv1 with conv1_bn folded as [27][C] float32 (gpp_mobilenet_stem), and per block the depthwise kernel with its BN
        folded as [9][C] float32 + bias, the pointwise kernel with its BN folded, packed for the arithmetic mode (layers/mobilenet.py) """
        torch, dev, eps = self.torch, self.device, W.MOBILENET_BN_EPSILON

        def up(a):
            return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev).contiguous()
        k, b = W.folded_conv(weights, 'conv1', 'conv1_bn', eps=eps)
        self.stem_w, self.stem_b = up(k.reshape(27, k.shape[3])), up(b)
        self.mbn_w = {}
        for i, cin, cout, _ in W.mobilenet_blocks(self.backbone_name):
            dw = {'dw/kernel': np.transpose(weights['conv_dw_{}/depthwise_kernel'.format(i)], (0, 1, 3, 2))}      # (3, 3, 1, C): C as outputs
            dw.update({'bn/' + p: weights['conv_dw_{}_bn/{}'.format(i, p)] for p in ('gamma', 'beta', 'moving_mean', 'moving_variance')})
            kd, bd = W.folded_conv(dw, 'dw', 'bn', eps=eps)
            kp, bp = W.folded_conv(weights, 'conv_pw_{}'.format(i), 'conv_pw_{}_bn'.format(i), eps=eps)
            pw, scale = M.pack_pointwise(kp, self.dtype, dev)
            self.mbn_w[i] = (up(M.pack_depthwise(np.transpose(kd, (0, 1, 3, 2)))), up(bd), pw, up(bp), scale)

    # ------------------------------------------------------------------ plan
    def _plan_options(self, B):
        """ every GPP_* switch of the plan builder as its effective value for this model and batch (models/plan.py) """
        return plan_options(self, B)

    def _build(self, B, H, Wd, n_planes, planes_batched, ragged=False):
        """ ragged: the plan of a height class (utils/image.py) -- H = 4 Hp is the row count of the canvas, and the stem and pool1 take
        every image's own height from plan.heights (int32, on the device: data of the plan, so one plan and one captured graph serve
        every mix of heights); everything behind pool1 is the uniform plan's """
        if ragged:
            if self.mobilenet or self.densenet:
                raise ValueError('{} has no ragged form: {}; run its images grouped by shape'.format(
                    self.backbone_name, 'its first block runs at conv1\'s resolution, which differs inside a height class' if self.mobilenet
                    else 'its zero-padded pool1 (gpp_maxpool3x3s2_pad_f32) has no per-image form'))
            if self.audit:
                raise ValueError('range_audit=True has no ragged form: the audit of the conv1 map reads rows that a shorter image does not have')
            if H % 4:
                raise ValueError('the canvas of a ragged plan has 4 Hp rows, got {}'.format(H))
        builder = PlanBuilder(self, B, H, Wd, n_planes, planes_batched, ragged)
        plan = builder.build()
        if builder.opts.autotune:
            self._autotune(plan)
        return plan

    def _autotune(self, plan):
        """ the tile of every layer of the plan, timed on the device or remembered (models/tuning.py) """
        tuning.autotune(self, plan)

    def x3_range_events(self, reset=False):
        """ dtype='f16x3': how many 8-channel groups the epilogues of THIS model's plans have stored with a value outside the half range (a finite
        activation beyond +-65504, which is clamped, or an inf / NaN, which stays one) since the counters were last reset.  Every plan counts
        into a slot of its own (Plan.range_slot): other models on the device, other plans and their resets do not show here, and a reset here
        touches nothing of theirs.  Zero = the type's range altered nothing.  Synchronises. """
        if self.dtype != 'f16x3':
            return 0
        self.torch.cuda.synchronize()
        total = 0
        for plan in self._plans.values():
            total += int(plan.range_slot.item())
            if reset:
                plan.range_slot.zero_()
                plan.range_seen = 0
        if reset:
            self.torch.cuda.synchronize()
        return total

    def note_range(self, plan, count):
        """ count = the plan's counter as a fetched result saw it: True when events happened since the plan's previous fetch """
        if count == plan.range_seen:
            return False
        plan.range_seen = count
        return True

    def plan_for(self, B, H, Wd, n_planes, planes_batched, ragged=False):
        """ ragged=True: the plan of the height class whose canvas has H = 4 Hp rows (key: the class in place of H) """
        key = (int(B), int(H), int(Wd), int(n_planes), bool(planes_batched))
        if ragged:
            key = (key[0], ('class', key[1] // 4), key[2], key[3], key[4])
        if key not in self._plans:
            self._plans[key] = self._build(int(B), int(H), *key[2:], **({'ragged': True} if ragged else {}))
        self._last_plan = self._plans[key]
        return self._plans[key]

    def put_heights(self, plan, heights):
        """ the image heights of the next run of a ragged plan into its device table (asynchronous).  The library cannot read the table,
        so the range is checked here: every height must lie in the plan's class, [4 Hp - 3, 4 Hp]. """
        from ..utils import image as image_utils
        if not getattr(plan, 'ragged', False):
            raise ValueError('put_heights: not a ragged plan')
        B, rows = plan.shape[0], plan.shape[1]
        lo, hi = image_utils.class_height_range(rows // 4)
        h = [int(v) for v in np.asarray(heights).reshape(-1)]
        if len(h) != B or any(v < lo or v > hi for v in h):
            raise ValueError('heights {} do not fit the plan: {} images of height {}..{} (class Hp = {})'.format(h, B, lo, hi, rows // 4))
        plan.heights_host = h
        plan.heights.copy_(self.torch.as_tensor(np.asarray(h, dtype=np.int32)), non_blocking=True)

    # ------------------------------------------------------------------ execution
    def _require_hip(self):          # a model built on another device (the CPU plan tests): its plans can be inspected, never run
        if self.device.type != 'cuda':
            raise hip.GppError('the model was built on {}: its plans do not run'.format(self.device))

    def run_op(self, plan, index):
        """ Enqueue ONE op of the plan (per-layer tests). """
        self._require_hip()
        hip.check(hip.lib().gpp_plan_run(ctypes.byref(plan.array, index * ctypes.sizeof(PlanOp)), 1, hip.stream_ptr(), None, 0), 'gpp_plan_run')
        kind, _, desc, name, _ = plan.ops[index]
        if kind == OP_CONV and desc.lists_after:
            # the op has made the deep lists and set their flags; an op run on its own writes its whole map, so the
            # flags are 1 again behind it, ordered on the stream
            plan.sparse.reset_deep()
        if kind == OP_CONV and name == TOWER0 and plan.sparse is not None and plan.sparse.tower0 is not None:
            # the plan's launch under this name computes the columns behind the regression slice (PlanBuilder.towers_0_split); an op run
            # on its own writes its whole map: the slice dense, here
            d = type(plan.sparse.tower0).from_buffer_copy(plan.sparse.tower0)
            d.deep_rows = d.deep_counts = d.deep_flag = None
            d.deep_tile = 0
            hip.check(hip.lib().gpp_conv2d_igemm(ctypes.byref(d), hip.stream_ptr()), 'gpp_conv2d_igemm (regression slice of {})'.format(TOWER0))

    def run_plan(self, plan, events=None):
        """ Enqueue the whole forward on the current stream (asynchronous). """
        self._require_hip()
        plan.heads_stale = plan.sparse is not None
        if events is None and getattr(plan, 'graph', None) is not None:
            plan.graph.replay()
            return
        if events is not None:
            arr = (ctypes.c_void_p * len(events))(*events)
            rc = hip.lib().gpp_plan_run(plan.array, len(plan.ops), hip.stream_ptr(), arr, len(events))
        else:
            rc = hip.lib().gpp_plan_run(plan.array, len(plan.ops), hip.stream_ptr(), None, 0)
        hip.check(rc, 'gpp_plan_run')

    def capture(self, plan):
        """ Record the plan into a HIP graph (via torch's stream capture); later run_plan(plan) calls replay
        it with one launch.  Measured on MI355X: no gain (B = 1: 2.00 -> 1.98 ms, B = 8: 5.44 -> 5.43 ms) -- the plan
        is GPU-bound, kernel time is 99 % of the step -- so it is optional and off by default. """
        self._require_hip()
        torch = self.torch
        self.run_plan(plan)                      # warm-up outside the capture (one-time kernel attribute calls)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        plan.heads_stale = plan.sparse is not None
        with torch.cuda.graph(graph):
            rc = hip.lib().gpp_plan_run(plan.array, len(plan.ops), hip.stream_ptr(), None, 0)
        hip.check(rc, 'gpp_plan_run (capture)')
        plan.graph = graph
        return graph

    def outputs(self, plan):
        """ the 8 device tensors in the reference's output order (retinanet.py:418-419) """
        return [plan.boxes, plan.dimensions, plan.scores, plan.labels, plan.orientations,
                plan.keypoints, plan.keyplanes, plan.residuals]

    def predict_on_batch(self, inputs):
        """ inputs = [images (B, H, W, 3) float32 BGR mean-subtracted, P_inv (B, 4, 3), planes (B, N, 4)]
        (NumPy, as bin/run_network.py:105 builds them, or torch tensors already on the device).
        Returns the list of 8 writable NumPy arrays of the reference:
        boxes (B,100,12) f32, dimensions (B,100,3) f32, scores (B,100) f32, labels (B,100) i32,
        orientations (B,100) i32, keypoints (B,100,4,3) f32, keyplanes (B,100,1,4) f32, residuals (B,100) f32. """
        plan = self.stage_inputs(inputs)
        self.run_plan(plan)
        return self.fetch(plan)

    def fetch(self, plan, packed=None):
        """ the 8 result arrays of the plan's last run as writable NumPy arrays (synchronises).  packed (default; GPP_FETCH=separate for
        the other form): ONE launch packs them into a (B, 100, 35) float32 tensor (gpp_pack_detections; labels / orientations are small
        integers: exact) and ONE copy brings it to the host, instead of eight blocking copies of 0.4 - 4.8 KB per image -- the same bytes
        (tests/test_network_gpu.py), 8 -> 1 host round trips inside the bracket the reference times (bin/run_network.py:108-111). """
        return self._answer(plan, 'predict_on_batch', self.outputs_reader(packed))

    @staticmethod
    def outputs_reader(packed=None):
        """ how fetch reads the 8 arrays (a reader of _answer): packed, the counter rides behind the detections (pack_with_range); the
        other form makes eight copies and reads an 8-byte snapshot behind them """
        if packed is None:
            packed = os.environ.get('GPP_FETCH', 'packed') != 'separate'
        if packed:
            return lambda model, plan: model.unpack_with_range(model.pack_with_range(plan).cpu().numpy(), plan.shape[0])
        return RetinaNet3D.behind_snapshot(lambda model, plan: [t.cpu().numpy() for t in model.outputs(plan)])

    # ------------------------------------------------------------------ f16x3: the lower range, audited (range_audit=True)
    def range_audit(self, plan=None):
        """ range_audit=True: the report of the plan's last run (default: the plan of the last call), one record per audited map, from ONE
        copy of the plan's abs-max table (synchronises): see audit_report for the fields and for what `flagged` does and does not say """
        if not self.audit:
            raise hip.GppError('this model keeps no range audit: load it with range_audit=True (models.load_model(..., range_audit=True))')
        plan = plan or self._last_plan
        if plan is None:
            raise hip.GppError('range_audit: no plan has run yet')
        return audit_report(plan.audit_maps, plan.audit_table.cpu().numpy())

    def range_audit_unobserved(self, plan=None):
        """ the x3 operands of the plan that a pass over HBM cannot see, [{name, consumers, reason}]: listed, not dropped silently """
        plan = plan or self._last_plan
        return [{k: u[k] for k in ('name', 'consumers', 'reason')} for u in plan.audit_unobserved]

    def _audit_flags(self, plan):
        """ an audit model's synchronous calls: read the table of the run just fetched (the one extra copy this mode accepts), keep the
        report (last_range_audit; plan.audit_flagged = its flagged maps), count them; returns those the call has to react to ([] for
        on_range_event='ignore' and for other models).  A run that left the half range is not audited: both keep the previous call's """
        if not self.audit:
            return []
        self.last_range_audit = self.range_audit(plan)
        plan.audit_flagged = [r for r in self.last_range_audit if r['flagged']]
        self.small_magnitude_events += len(plan.audit_flagged)
        return plan.audit_flagged if self.on_range_event != 'ignore' else []

    @staticmethod
    def _small_magnitude_message(what, flagged):
        return ('{}: the largest value of {} lies below 2^-9, where the IEEE-half pair of dtype=\'f16x3\' is a fixed-point number (quantum '
                '2^-24) that keeps fewer than 16 bits of it: the result would not be the reference\'s -- load the model with dtype=\'f32\' '
                'or on_range_event=\'f32\''.format(what, ', '.join('the map behind {} (read by {}; max {:.3g})'.format(
                    r['name'], ', '.join(r['consumers']), r['absmax']) for r in flagged)))

    # ------------------------------------------------------------------ f16x3: the half range, watched
    def watches_range(self):
        return self.dtype == 'f16x3' and self.on_range_event != 'ignore'

    def range_snapshot(self, plan, dst=None):
        """ enqueue a copy of the plan's range-event counter (its value at this point of the current stream) into two float32 words
        of device memory (gpp_x3_range_snapshot_of); no synchronisation """
        if dst is None:
            dst = self.torch.empty((2,), dtype=self.torch.float32, device=self.device)
        hip.check(hip.lib().gpp_x3_range_snapshot_of(ctypes.c_void_p(plan.range_slot.data_ptr()), ctypes.c_void_p(dst.data_ptr()), hip.stream_ptr()),
                  'gpp_x3_range_snapshot_of')
        return dst

    def pack_with_range(self, plan, out=None):
        """ the results of the plan's last run as ONE flat float32 device buffer: B x 100 x 35 packed detections (gpp_pack_detections)
        followed by the 8 bytes of the range-event counter as the stream saw it behind them -- one copy brings both to the host """
        from ..utils import distributed as D
        torch = self.torch
        outs = self.outputs(plan)
        B, Dn = int(outs[0].shape[0]), int(outs[0].shape[1])
        n = B * Dn * D.PACK_WIDTH
        if out is None:
            out = torch.empty((n + 2,), dtype=torch.float32, device=self.device)
        hip.check(hip.lib().gpp_pack_detections(*([hip.ptr(o) for o in outs] + [B, Dn, ctypes.c_void_p(out.data_ptr()), hip.stream_ptr()])),
                  'gpp_pack_detections')
        if self.watches_range():
            self.range_snapshot(plan, out[n:])
        return out

    @staticmethod
    def unpack_with_range(flat, B):
        """ host side of pack_with_range: (the 8 NumPy result arrays, the counter value) """
        from ..utils import distributed as D
        flat = np.ascontiguousarray(flat)
        n = flat.size - 2
        return D.unpack_outputs(flat[:n].reshape(B, n // (B * D.PACK_WIDTH), D.PACK_WIDTH)), int(flat[n:].view(np.uint64)[0])

    # One path from a plan that has just been enqueued to an answered call.  A *reader* is what a call supplies: reader(model, plan) ->
    # (the call's result read from that plan, the plan's range counter as the stream saw it behind the result) -- the counter comes with
    # the copy the call makes anyway (pack_with_range, fetch_poses) or as 8 bytes of its own (behind_snapshot), never with a further
    # synchronisation; a model that does not watch the range returns any number there.  Everything else happens here, once.
    @staticmethod
    def behind_snapshot(result_of):
        """ a reader for a result that does not carry the counter itself: the 8-byte snapshot (range_snapshot) is enqueued in front of
        result_of(model, plan) and read behind it """
        def reader(model, plan):
            snapshot = model.range_snapshot(plan) if model.watches_range() else None
            result = result_of(model, plan)
            return result, 0 if snapshot is None else int(snapshot.cpu().view(model.torch.int64).item())
        return reader

    def _answer(self, plan, what, reader, restage=None):
        """ the result of the plan's run for the call `what`: the reader's, unless an activation of the run left the half range or (an
        audit model; looked at only when the range held) a whole map sits below it -- then what _range_event returns """
        result, count = reader(self, plan)
        self._answered = (self, plan)
        event = self.watches_range() and self.note_range(plan, count)
        flagged = [] if event else self._audit_flags(plan)
        if event or flagged:
            return self._range_event(plan, what, reader, flagged, restage)
        return result

    def _range_event(self, plan, what, reader, flagged=(), restage=None):
        """ the run of `plan` just read is not the reference's (note_range said so, or `flagged` names the maps of an audit model): count
        it, then raise, or run the call again on the float32 twin and read the same thing there.  The twin gets the call's inputs where
        they still are: the plan's images (a ragged plan: its canvas and heights), P_inv, planes and frame_info in HBM -- or what
        restage(twin) -> its plan stages (FramePipeline: the slot's raw frames).  Everything is enqueued on the current stream.
        utils/pipeline.py and utils/distributed.py come here behind their own note_range. """
        self.range_fallbacks += 1
        if self.on_range_event == 'raise' and flagged:
            raise hip.GppError(self._small_magnitude_message(what, flagged))
        if self.on_range_event == 'raise':
            raise hip.GppError('{}: an activation left the IEEE-half range of dtype=\'f16x3\' (finite beyond +-65504, inf or NaN; '
                               'gpp_x3_range_events): the result would not be the reference\'s -- load the model with dtype=\'f32\' '
                               'or on_range_event=\'f32\''.format(what))
        twin = self.prepare_fallback()
        if restage is not None:
            twin_plan = restage(twin)
        else:
            inputs = [plan.images, plan.P_inv, plan.planes]
            twin_plan = twin.stage_canvas(inputs, plan.heights_host) if plan.ragged else twin.stage_inputs(inputs)
        if self.pose:
            twin_plan.frame_info.copy_(plan.frame_info)          # (what put_frame_info gave the call, or the plan's default)
        twin.run_plan(twin_plan)
        self._answered = (twin, twin_plan)
        return reader(twin, twin_plan)[0]

    def prepare_fallback(self, B=None, H=None, Wd=None, n_planes=None, planes_batched=True, ragged=False):
        """ on_range_event='f32': build the float32 twin NOW -- its weights upload (a second copy of the weights in HBM) and, when a shape is
        given, its plan for that shape (buffers + tile tuning: seconds) -- instead of inside the first call whose activations leave the half
        range, where it would stall a latency-critical predict_on_batch / FramePipeline iteration (and every other rank of a sharded call).
        Without it the twin is built lazily, at the first event.  The host copy of the weights is dropped once the twin exists. """
        if self.dtype != 'f16x3' or self.on_range_event != 'f32':
            return None
        if self._twin is None:
            self._twin = RetinaNet3D(self._weights, backbone_name=self.backbone_name, dtype='f32', nms=self.nms,
                                     class_specific_filter=self.class_specific_filter, orientation_specific_filter=self.osf,
                                     name=self.name + '-f32-twin', plan=self.plan_mode, pose=self.pose, cuboid_nms=self.cuboid_nms)
            self._weights = None
        if B is not None:
            self._twin.plan_for(B, H, Wd, n_planes, planes_batched, ragged=ragged)
        return self._twin

    def stage_inputs(self, inputs):
        """ Copy [images, P_inv, planes] into the plan's device buffers; returns the plan. """
        torch = self.torch
        if not isinstance(inputs, (list, tuple)) or len(inputs) != 3:
            raise ValueError('predict_on_batch expects [images, P_inv, planes]')
        images, P_inv, planes = inputs
        if isinstance(images, (list, tuple)):
            return self._stage_ragged_images(images, P_inv, planes)
        shp = tuple(images.shape)
        if len(shp) != 4 or shp[3] != 3:
            raise ValueError('images must be (B, H, W, 3), got {}'.format(shp))
        n_planes, batched = self._check_calibration(shp[0], P_inv, planes)
        plan = self.plan_for(shp[0], shp[1], shp[2], n_planes, batched)
        if not isinstance(images, torch.Tensor) and os.environ.get('GPP_UPLOAD', 'pageable') == 'pinned':
            # GPP_UPLOAD=pinned: host frames go through a page-locked staging buffer of the plan (one memcpy on the host, then a DMA).
            # Measured at batch 1 (tools/b1_latency.py --host-variants, profiles/r5/b1_latency.json): 0.37 ms for the 6.4 MB float32 frame
            # against 0.16 - 0.17 ms for the runtime's own staged copy from pageable memory -- the host memcpy costs more than it saves,
            # so the plain copy is the default
            if getattr(plan, 'host_images', None) is None:
                plan.host_images = torch.empty(tuple(plan.images.shape), dtype=torch.float32, pin_memory=True)
                plan.host_images_free = torch.cuda.Event()
            else:
                plan.host_images_free.synchronize()          # the previous upload out of this buffer has left it
            np.copyto(plan.host_images.numpy(), images, casting='same_kind')
            plan.images.copy_(plan.host_images, non_blocking=True)
            plan.host_images_free.record()
        else:
            self._put(plan.images, images)
        self._put(plan.P_inv, P_inv)
        self._put(plan.planes, planes)
        return plan

    # ------------------------------------------------------------------ ragged batches: images of one height class, different heights
    @property
    def supports_ragged(self):
        """ predict_on_batch / predict_on_frames / predict_poses_on_frames take a LIST of images of one height class (the ResNets; not
        with range_audit=True) """
        return not (self.mobilenet or self.densenet or self.audit)

    @staticmethod
    def _check_calibration(B, P_inv, planes):
        if tuple(P_inv.shape) != (B, 4, 3):
            raise ValueError('P_inv must be (B, 4, 3), got {}'.format(tuple(P_inv.shape)))
        pshape = tuple(planes.shape)
        batched = len(pshape) == 3
        if not ((batched and pshape[0] == B and pshape[2] == 4) or (len(pshape) == 2 and pshape[1] == 4)) or pshape[-2] < 1:
            raise ValueError('planes must be (B, N, 4) or (N, 4), got {}'.format(pshape))
        return pshape[-2], batched

    def _put(self, dst, src):
        """ the one copy into a plan's buffer: a device tensor or a host array (asynchronous) """
        torch = self.torch
        src_t = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(src, dtype=np.float32))
        dst.copy_(src_t.to(dtype=dst.dtype), non_blocking=True)

    def stage_canvas(self, inputs, heights):
        """ stage_inputs for a ragged batch that is already a canvas: inputs = [canvas (B, 4 Hp, W, 3) float32 with image b in rows
        [0, heights[b]) of slot b, P_inv, planes]; returns the ragged plan of the class """
        canvas, P_inv, planes = inputs
        shp = tuple(canvas.shape)
        if len(shp) != 4 or shp[3] != 3 or shp[1] % 4:
            raise ValueError('the canvas must be (B, 4 Hp, W, 3), got {}'.format(shp))
        n_planes, batched = self._check_calibration(shp[0], P_inv, planes)
        plan = self.plan_for(shp[0], shp[1], shp[2], n_planes, batched, ragged=True)
        self.put_heights(plan, heights)
        self._put(plan.images, canvas)
        self._put(plan.P_inv, P_inv)
        self._put(plan.planes, planes)
        return plan

    def _stage_ragged_images(self, images, P_inv, planes):
        """ images: a list of (H_i, W, 3) float32 arrays (NumPy or torch) of ONE height class -> the canvas and the heights of its plan """
        from ..utils import image as image_utils
        torch = self.torch
        shapes = [tuple(im.shape) for im in images]
        if not shapes or any(len(s) != 3 or s[2] != 3 for s in shapes):
            raise ValueError('a ragged batch is a non-empty list of (H, W, 3) images, got shapes {}'.format(shapes))
        classes = sorted(set(image_utils.class_of_resized(s[0], s[1]) for s in shapes))
        if len(classes) != 1:
            raise ValueError('the images span {} height classes (Hp, W): {}: a ragged batch holds one class '
                             '(utils.image.split_by_height_class groups a list)'.format(len(classes), ' and '.join(str(c) for c in classes)))
        (Hp, Wd), B = classes[0], len(shapes)
        if all(isinstance(im, torch.Tensor) for im in images):
            canvas = torch.zeros((B, 4 * Hp, Wd, 3), dtype=torch.float32, device=images[0].device)
            for b, im in enumerate(images):
                canvas[b, :shapes[b][0]] = im
        else:
            canvas = np.zeros((B, 4 * Hp, Wd, 3), np.float32)
            for b, im in enumerate(images):
                canvas[b, :shapes[b][0]] = im.cpu().numpy() if isinstance(im, torch.Tensor) else im
        return self.stage_canvas([canvas, P_inv, planes], [s[0] for s in shapes])

    def _stage_ragged_frames(self, frames, P_inv, planes, min_side, max_side):
        """ frames: a list of (h_i, w_i, 3) uint8 frames that resize into ONE height class: uploads the raw bytes (frame b densely at the
        start of slot b of a uint8 canvas of the largest raw size) and preprocesses them into the plan's canvas on the device
        (gpp_preprocess_u8_bgr_ragged, per-image taps).  Returns (plan, scales (B,)). """
        from ..utils import image as image_utils
        torch, dev = self.torch, self.device
        frames = [f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames]
        if not frames or any(f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 for f in frames):
            raise ValueError('a ragged batch of frames is a non-empty list of (h, w, 3) uint8 frames')
        shapes = tuple(self._frame_shapes(frames))
        (Hp, Wo), heights, scales, taps = image_utils.ragged_taps(shapes, min_side, max_side)      # (ValueError: more than one class)
        B, Hr, Wr = len(frames), max(s[0] for s in shapes), max(s[1] for s in shapes)
        n_planes, batched = self._check_calibration(B, P_inv, planes)
        key = (shapes, min_side, max_side)
        if key not in self._ragged_taps:
            self._ragged_taps[key] = [torch.as_tensor(a).to(dev) for a in taps] + [torch.as_tensor(np.asarray(shapes, dtype=np.int32)).to(dev)]
        y0, y1, wy, x0, x1, wx, raw_hw = self._ragged_taps[key]
        plan = self.plan_for(B, 4 * Hp, Wo, n_planes, batched, ragged=True)
        self.put_heights(plan, heights)
        raw = np.zeros((B, Hr * Wr * 3), np.uint8)
        for b, f in enumerate(frames):
            raw[b, :f.size] = f.reshape(-1)
        frames_d = torch.as_tensor(raw).to(dev, non_blocking=True)
        m = image_utils.IMAGENET_MEAN_BGR
        hip.check(hip.lib().gpp_preprocess_u8_bgr_ragged(hip.ptr(frames_d), hip.ptr(plan.images), hip.ptr(raw_hw), hip.ptr(plan.heights),
                                                         hip.ptr(y0), hip.ptr(y1), hip.ptr(wy), hip.ptr(x0), hip.ptr(x1), hip.ptr(wx),
                                                         B, Hr, Wr, Hp, 4 * Hp, Wo, float(m[0]), float(m[1]), float(m[2]), hip.stream_ptr()),
                  'gpp_preprocess_u8_bgr_ragged')
        self._put(plan.P_inv, P_inv)
        self._put(plan.planes, planes)
        plan.keep_frames = frames_d
        return plan, np.asarray(scales, dtype=np.float64)

    # ------------------------------------------------------------------ raw frames (GPU preprocessing)
    def stage_frames(self, frames_u8, P_inv, planes, min_side=800, max_side=1333):
        """ frames_u8 (B, H, W, 3) uint8 BGR as utils.image.read_image_bgr returns them.  Uploads the raw
        bytes and runs mean subtraction + bilinear resize on the device (csrc/preprocess.hip), i.e. what
        bin/run_network.py:95-99 does on the host.  Returns (plan, scale). """
        from ..utils import image as image_utils
        torch = self.torch
        if isinstance(frames_u8, (list, tuple)):          # frames of one height class, different sizes: (plan, scales (B,))
            return self._stage_ragged_frames(frames_u8, P_inv, planes, min_side, max_side)
        frames = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frames_u8))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError('frames must be (B, H, W, 3) uint8, got {} {}'.format(tuple(frames.shape), frames.dtype))
        B, H, Wd = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        scale = image_utils.compute_resize_scale((H, Wd, 3), min_side, max_side)
        Ho, Wo = int(np.rint(H * scale)), int(np.rint(Wd * scale))
        key = (H, Wd, Ho, Wo)
        if key not in self._taps:
            y0, y1, wy = image_utils._axis_taps(Ho, H, scale)
            x0, x1, wx = image_utils._axis_taps(Wo, Wd, scale)
            dev = self.device
            self._taps[key] = [torch.as_tensor(a.astype(np.int32)).to(dev) for a in (y0, y1)] + [torch.as_tensor(wy).to(dev)] + \
                              [torch.as_tensor(a.astype(np.int32)).to(dev) for a in (x0, x1)] + [torch.as_tensor(wx).to(dev)]
        y0, y1, wy, x0, x1, wx = self._taps[key]
        n_planes, batched = self._check_calibration(B, P_inv, planes)
        plan = self.plan_for(B, Ho, Wo, n_planes, batched)
        frames_d = frames.to(self.device, non_blocking=True).contiguous()
        m = image_utils.IMAGENET_MEAN_BGR
        hip.check(hip.lib().gpp_preprocess_u8_bgr(hip.ptr(frames_d), hip.ptr(plan.images), hip.ptr(y0), hip.ptr(y1), hip.ptr(wy),
                                                  hip.ptr(x0), hip.ptr(x1), hip.ptr(wx), B, H, Wd, Ho, Wo,
                                                  float(m[0]), float(m[1]), float(m[2]), hip.stream_ptr()), 'gpp_preprocess_u8_bgr')
        self._put(plan.P_inv, P_inv)
        self._put(plan.planes, planes)
        plan.keep_frames = frames_d
        return plan, scale

    def predict_on_frames(self, frames_u8, P_inv, planes):
        """ predict_on_batch for raw uint8 BGR frames; returns (the 8 output arrays, scale).  P_inv must
        have been computed for that scale (utils.image.compute_resize_scale). """
        plan, scale = self.stage_frames(frames_u8, P_inv, planes)
        self.run_plan(plan)
        return self.fetch(plan), scale

    # ------------------------------------------------------------------ evaluation: detections matched to labels on the device
    def match_outputs(self, outputs, scales, annotations, iou_threshold=0.5, score_threshold=0.05, max_detections=100, num_classes=1):
        """ The matching of utils.eval.evaluate for one batch, on the device (csrc/eval.hip; one launch on the
        current stream).  outputs: the decode outputs on the device (boxes, dimensions, scores, labels, orientations[, ...]: the first five
        of `outputs(plan)`, or tensors made from stored results); scales: one per image (or one for all); annotations: per image the
        (n, 17) rows of KittiGenerator.load_annotations.  Returns four NumPy arrays (synchronises): table (B, D, 3) int32 -- bin, hit,
        annotation row of every detection, -1 where it is not selected --, scores (B, D) float32, errors (B, D, 11) float64, counts (B,)
        int32 (include/gpp.h, gpp_eval_match_f32); utils.eval.assemble_matches turns them into evaluate's result. """
        torch = self.torch
        boxes, dims, scores, labels, orientations = outputs[:5]
        B = int(scores.shape[0])
        if len(annotations) != B:
            raise ValueError('match_outputs: {} annotation arrays for {} images'.format(len(annotations), B))
        rows = [np.asarray(a, dtype=np.float64).reshape(-1, hip.GPP_EVAL_ANN_COLS) for a in annotations]
        padded = np.zeros((B, max(r.shape[0] for r in rows), hip.GPP_EVAL_ANN_COLS), np.float64)
        for b, r in enumerate(rows):
            padded[b, :r.shape[0]] = r
        dev = scores.device
        ann_d = torch.as_tensor(padded).to(dev, non_blocking=True)
        cnt_d = torch.as_tensor(np.asarray([r.shape[0] for r in rows], dtype=np.int32)).to(dev, non_blocking=True)
        scales_d = torch.as_tensor(np.array(np.broadcast_to(np.asarray(scales, dtype=np.float64).reshape(-1), (B,)), dtype=np.float32)).to(dev, non_blocking=True)
        table, errors, counts = hip.eval_match(boxes, dims, scores, labels, orientations, scales_d, ann_d, cnt_d, num_classes,
                                               score_threshold, max_detections, iou_threshold)
        return table.cpu().numpy(), scores.cpu().numpy(), errors.cpu().numpy(), counts.cpu().numpy()

    def match_on_frames(self, frames_u8, P_inv, planes, annotations, iou_threshold=0.5, score_threshold=0.05, max_detections=100, num_classes=1,
                        min_side=800, max_side=1333):
        """ predict_on_frames + match_outputs without the detour over the host: frames_u8 a (B, H, W, 3) uint8 BGR array or a list of
        frames of one height class, staged as predict_on_frames stages them (stage_frames: P_inv must have been computed for the scale
        that min_side / max_side give); the match launch follows the plan on its stream, and only
        table, scores, errors and counts come back.  Returns ((table, scores, errors, counts), scale).  When an activation leaves the
        half range of dtype='f16x3' the float32 twin answers the call, as it does for predict_on_frames. """
        self._require_hip()
        plan, scale = self.stage_frames(frames_u8, P_inv, planes, min_side, max_side)
        self.run_plan(plan)
        args = (scale, annotations, iou_threshold, score_threshold, max_detections, num_classes)
        reader = self.behind_snapshot(lambda model, p: model.match_outputs(model.outputs(p), *args))
        return self._answer(plan, 'match_on_frames', reader), scale

    # ------------------------------------------------------------------ pose rows (pose=True)
    def _require_pose(self):
        if not self.pose:
            raise hip.GppError('this model has no pose stage: load it with pose=True (models.load_model(..., pose=True))')

    def put_frame_info(self, plan, scales, image_shapes):
        """ (scale, raw height, raw width) of every image of the batch into the plan's frame_info buffer (asynchronous) """
        B = plan.shape[0]
        info = np.empty((B, 3), np.float32)
        info[:, 0] = np.asarray(scales, dtype=np.float64).reshape(-1)                       # one scale, or one per image
        info[:, 1:] = np.asarray(image_shapes, dtype=np.float64).reshape(-1, len(np.atleast_2d(image_shapes)[0]))[:, :2]
        plan.frame_info.copy_(self.torch.as_tensor(info), non_blocking=True)

    @staticmethod
    def _frame_shapes(frames_u8):
        """ the raw (h, w) of every frame of either form of frames_u8: a list of frames, or one (B, h, w, 3) array """
        if isinstance(frames_u8, (list, tuple)):
            return [tuple(int(v) for v in f.shape[:2]) for f in frames_u8]
        return [tuple(int(v) for v in frames_u8.shape[1:3])] * int(frames_u8.shape[0])

    def cuboid_suppressors(self):
        """ cuboid_nms=(metric, threshold): the (B, 100) int32 suppressor table of the last answered call -- for every row the index of
        the kept row that removed it, -1 for kept rows and padding (include/gpp.h, gpp_cuboid_nms_f64); the float32 twin's when it
        answered the call.  One copy (synchronises). """
        if self.cuboid_nms is None:
            raise hip.GppError('this model has no cuboid NMS stage: load it with pose=True, cuboid_nms=(metric, threshold)')
        if self._answered is None:
            raise hip.GppError('cuboid_suppressors: no call has been answered yet')
        return self._answered[1].pose_suppressor.cpu().numpy()

    def fetch_poses(self, plan, what='predict_poses_on_batch'):
        """ (rows (B, 100, 36) float32, counts (B,) int32) of the plan's last run, as fetch returns the 8 arrays: one copy (synchronises);
        the float32 twin's after a range event """
        return self._answer(plan, what, self.read_poses)

    @staticmethod
    def read_poses(model, plan):
        """ the reader of fetch_poses: ONE copy of pose_out brings the rows, the range counter behind them and the counts """
        n = plan.pose_rows.numel()
        if model.watches_range():
            model.range_snapshot(plan, plan.pose_out[n:n + 2])
        flat = plan.pose_out.cpu().numpy()
        rows, counts = flat[:n].reshape(tuple(plan.pose_rows.shape)).copy(), flat[n + 2:].view(np.int32).copy()
        return (rows, counts), int(flat[n:n + 2].view(np.uint64)[0])

    def predict_poses_on_batch(self, inputs, scales, image_shapes, heights=None):
        """ predict_on_batch + what bin/run_network.py does with its result on the host, on the device: inputs as predict_on_batch;
        scales: the image scale of every image (or one for all); image_shapes: the raw images' (height, width[, 3]) (or one for all).
        Returns (rows (B, 100, 36) float32 -- include/gpp.h, gpp_pose_f32 --, counts (B,) int32: the detections above the score
        threshold, which are the first counts[b] rows of image b).  utils.gpp_utils.detections_from_rows / kitti_lines_from_rows
        turn one image's rows into the dict of recover_pose / the KITTI text.
        A cuboid_nms model: the rows a kept row suppressed are -1 throughout WHERE THEY STOOD (no compaction) and counts[b] is the number
        of kept rows -- the detections are the rows whose column 14 is >= 0; utils.cuboid_nms.live_first moves them to the front for the
        two readers above. """
        self._require_pose()
        plan = self.stage_inputs(inputs) if heights is None else self.stage_canvas(inputs, heights)      # (heights: inputs[0] is a ragged canvas)
        self.put_frame_info(plan, scales, image_shapes)
        self.run_plan(plan)
        return self.fetch_poses(plan)

    def predict_poses_on_frames(self, frames_u8, P_inv, planes):
        """ predict_poses_on_batch for raw uint8 BGR frames (predict_on_frames): returns ((rows, counts), scale) """
        self._require_pose()
        plan, scale = self.stage_frames(frames_u8, P_inv, planes)
        self.put_frame_info(plan, scale, self._frame_shapes(frames_u8))
        self.run_plan(plan)
        return self.fetch_poses(plan, 'predict_poses_on_frames'), scale

    # ------------------------------------------------------------------ tracks (pose=True, track=...)
    def _track_buffers(self):
        if self.track is None:
            raise hip.GppError('this model has no tracker: load it with pose=True, track=(metric, threshold)')
        if self._track_state is None:
            torch = self.torch
            state = torch.zeros((2, 1, hip.track_state_bytes()), dtype=torch.uint8, device=self.device)
            self._track_state = [state[0], state[1]]
            self._track_work = torch.empty((hip.track_workspace_bytes(1),), dtype=torch.uint8, device=self.device)
            self._track_params = track_utils.params_of(self.track)
            self._track_optimal = track_utils.is_optimal(self.track)     # 'assign': 'optimal' -> gpp_track_optimal_f64 (section 4.32)
            self._track_ego_work = None          # 'ego': True -> gpp_track_ego_f64 (section 4.33): (B, workspace), sized with the plan's B
            self._track_kf = track_utils.kf_params_of(self.track)        # 'filter': 'kalman' -> gpp_track_kf_f64 (section 4.34), or None
            if self._track_kf is not None:       # (its workspace is the ego form's, with or without records)
                cov = torch.zeros((2, 1, hip.track_cov_bytes()), dtype=torch.uint8, device=self.device)
                self._track_cov = [cov[0], cov[1]]
        return self._track_state

    def _track_ego(self, ego, frames, what):
        """ the `ego` argument of predict_tracks_on_*: None on a model without 'ego', the checked (B, 16) records on a model with it --
        a missing or a superfluous one is refused before anything is staged """
        wants = self.track is not None and self.track.get('ego', False)
        if wants and ego is None:
            raise hip.GppError("{}: this model compensates ego-motion (track={{..., 'ego': True}}): it needs ego=records, one per frame "
                               "(utils.track.ego_records, utils.oxts.camera_ego)".format(what))
        if not wants and ego is not None:
            raise hip.GppError("{}: ego records were given, but this model was not loaded with track={{..., 'ego': True}}".format(what))
        if ego is None:
            return None
        try:
            return track_utils.check_ego(ego, frames)
        except ValueError as e:
            raise hip.GppError('{}: {}'.format(what, e))

    def reset_tracks(self):
        """ start a new sequence: the empty tracker (the next birth gets id 0), and with 'filter': 'kalman' its zero covariances """
        self._track_buffers()[0].zero_()
        if self._track_cov is not None:
            self._track_cov[0].zero_()

    def track_state(self):
        """ the tracker's state as one utils.track.STATE_DTYPE record (include/gpp.h, gpp_track_state).  One copy (synchronises). """
        return track_utils.read_state(self._track_buffers()[0])[0]

    def track_covariance(self):
        """ the covariances that belong to track_state(), (10, 128) float64 -- utils.track.COV_FIELDS by slot (include/gpp.h,
        gpp_track_cov) -- on a model loaded with track={..., 'filter': 'kalman'}.  One copy (synchronises). """
        self._track_buffers()
        if self._track_cov is None:
            raise hip.GppError("this model's tracker keeps no covariance: load it with track={..., 'filter': 'kalman', 'noise': {...}}")
        return track_utils.read_cov(self._track_cov[0])[0]

    def fetch_tracks(self, plan, what='predict_tracks_on_batch', ego=None):
        """ ((rows, counts, ids, hits)) of the plan's last run: fetch_poses + the tracker's frame steps over the images of the batch, in
        order.  The launch follows the plan (and its cuboid NMS) on the stream and is no plan op; it goes from the current state to a
        second buffer, because _range_event calls the reader a second time on the float32 twin: the model commits by swapping the two
        only after _answer has returned -- the state advances once per answered call, by the rows that answered it.  ego: the checked
        (B, 16) records of an 'ego' model (_track_ego): the launch is gpp_track_ego_f64, and the twin's second call takes the same ones.
        With 'filter': 'kalman' the launch is gpp_track_kf_f64 and the covariances go the state's way: from the current buffer to a
        second one, swapped together with the states -- a range event advances both once. """
        torch = self.torch
        state, nxt = self._track_buffers()
        B, D = int(plan.pose_rows.shape[0]), int(plan.pose_rows.shape[1])
        work = self._track_work
        kf = self._track_kf
        cov, nxt_cov = self._track_cov if kf is not None else (None, None)
        if ego is not None or kf is not None:
            if self._track_ego_work is None or self._track_ego_work[0] != B:
                self._track_ego_work = (B, torch.empty((hip.track_ego_workspace_bytes(1, B),), dtype=torch.uint8, device=self.device))
            work = self._track_ego_work[1]
        smooth = self.track['smooth']
        out = torch.empty((B, D, hip.GPP_POSE_COLS), dtype=torch.float32, device=self.device) if smooth else None
        tags = torch.empty((2, B, D), dtype=torch.int32, device=self.device)

        def rows_and_tracks(model, p):
            # (smooth: the plan's rows stay what predict_poses_* reads; otherwise the kernel's bit copy lands where it came from)
            hip.track(p.pose_rows, state, self._track_params, state_out=nxt, out=out if smooth else p.pose_rows, ids=tags[0], hits=tags[1],
                      workspace=work, optimal=self._track_optimal, ego=ego, kf=kf, cov_in=cov, cov_out=nxt_cov)
            (rows, counts), count = self.read_poses(model, p)
            if smooth:
                rows = out.cpu().numpy()
            host = tags.cpu().numpy()
            return (rows, counts, host[0], host[1]), count

        result = self._answer(plan, what, rows_and_tracks)
        self._track_state = [nxt, state]
        if kf is not None:
            self._track_cov = [nxt_cov, cov]
        return result

    def predict_tracks_on_batch(self, inputs, scales, image_shapes, heights=None, ego=None):
        """ predict_poses_on_batch + the tracker: the images of the call are consecutive frames of the model's one sequence, a later call
        continues it (reset_tracks starts a new one).  Returns (rows (B, 100, 36) float32, counts (B,) int32, ids (B, 100) int32, hits
        (B, 100) int32): ids[b, d] is the identity of row d of image b, -1 for padding rows, rows with a NaN among their cuboid's fields
        and rows below the option's birth_score that matched nothing; hits the frames that identity has been seen in.  With smooth the
        cuboid's columns of rows that carry an id are the filter's (include/gpp.h, gpp_track_f64).  ego: on a model loaded with
        track={..., 'ego': True} the (B, 16) records of the frames (utils.track.ego_records; include/gpp.h, gpp_track_ego_f64) -- the
        first relates to the last frame of the call before; on any other model it must be None. """
        self._require_pose()
        self._track_buffers()
        ego = self._track_ego(ego, len(inputs[0]), 'predict_tracks_on_batch')
        plan = self.stage_inputs(inputs) if heights is None else self.stage_canvas(inputs, heights)
        self.put_frame_info(plan, scales, image_shapes)
        self.run_plan(plan)
        return self.fetch_tracks(plan, ego=ego)

    def predict_tracks_on_frames(self, frames_u8, P_inv, planes, ego=None):
        """ predict_tracks_on_batch for raw uint8 BGR frames (predict_on_frames): returns ((rows, counts, ids, hits), scale) """
        self._require_pose()
        self._track_buffers()
        ego = self._track_ego(ego, len(frames_u8), 'predict_tracks_on_frames')
        plan, scale = self.stage_frames(frames_u8, P_inv, planes)
        self.put_frame_info(plan, scale, self._frame_shapes(frames_u8))
        self.run_plan(plan)
        return self.fetch_tracks(plan, 'predict_tracks_on_frames', ego), scale

    def score_poses_on_frames(self, frames_u8, P_inv, planes, labels):
        """ predict_poses_on_frames + the overlaps of KITTI's object benchmark (csrc/kitti_eval.hip) without the
        detour over the host: frames_u8 a (B, H, W, 3) uint8 BGR array or a list of frames of one height class, staged as
        predict_poses_on_frames stages them; labels: per image the (n, 16) float64 rows of utils.kitti_eval.read_label_file (ORIGINAL
        label_2 lines).  The overlap launch follows the plan on its stream and reads the rows where the plan left them; nothing but the
        range watch's 8 bytes comes back.  Returns (chunk, scale): chunk a utils.kitti_eval.DeviceChunk -- this batch's rows (a copy: the
        plan's buffer is overwritten by its next run), labels, counts and overlaps on the device -- for utils.kitti_eval.evaluate_chunks,
        which runs the dataset-level passes over the chunks of all batches.  When an activation leaves the half range of dtype='f16x3'
        the float32 twin answers the call, as it does for match_on_frames: the chunk then holds the twin's rows and their overlaps. """
        self._require_pose()
        from ..utils import kitti_eval
        B = len(frames_u8)
        if len(labels) != B:
            raise ValueError('score_poses_on_frames: {} label arrays for {} frames'.format(len(labels), B))
        if max([np.asarray(g).reshape(-1, kitti_eval.LABEL_COLS).shape[0] for g in labels] + [0]) > hip.GPP_KITTI_MAX_LABELS:
            raise ValueError('score_poses_on_frames: an image has more than {} labels'.format(hip.GPP_KITTI_MAX_LABELS))
        plan, scale = self.stage_frames(frames_u8, P_inv, planes)
        self.put_frame_info(plan, scale, self._frame_shapes(frames_u8))
        self.run_plan(plan)
        reader = self.behind_snapshot(lambda model, p: kitti_eval.upload_chunk(p.pose_rows.clone(), labels, self.device))
        return self._answer(plan, 'score_poses_on_frames', reader), scale

    def predict_composites_on_frames(self, frames_u8, P_inv, planes, P_raw, score_threshold=0.4):
        """ predict_poses_on_frames + the pictures of bin/run_network.py --save-images, rendered on the device (csrc/draw.hip, DESIGN.md
        section 4.14): frames_u8 a (B, H, W, 3) uint8 array or a list of frames of one height class; P_raw (B, 3, 4) (or one (3, 4) for
        all): the calibration in raw-image pixels (reference run_network.py:115); detections with a score above score_threshold are drawn.
        Returns ((rows, counts), scale, [composite_b (2 h_b, w_b, 3) uint8]): the 2-D picture over the 3-D picture of every image, equal
        byte for byte to utils.visualization.composite_from_rows(frame_b, rows[b], counts[b], P_raw[b], score_threshold).
        The two draw launches follow the plan on its stream and are not plan ops; one more device -> host copy brings the pictures.  When
        the float32 twin answers the call (a range event), the rows and the pictures are the twin's, drawn over this call's frames. """
        self._require_pose()
        torch = self.torch
        plan, scale = self.stage_frames(frames_u8, P_inv, planes)
        shapes = self._frame_shapes(frames_u8)
        B = len(shapes)
        P_raw = np.array(np.broadcast_to(np.asarray(P_raw, dtype=np.float64), (B, 3, 4)))          # (a writable copy)
        self.put_frame_info(plan, scale, shapes)
        self.run_plan(plan)
        frames_d = plan.keep_frames                      # the raw bytes: image b densely at the start of slot b
        Hr, Wr = max(s[0] for s in shapes), max(s[1] for s in shapes)
        raw_hw = torch.as_tensor(np.asarray(shapes, dtype=np.int32)).to(self.device, non_blocking=True)
        P_d = torch.as_tensor(P_raw).to(self.device, non_blocking=True)
        slot = 2 * Hr * Wr * 3
        status_at = (B * slot + 15) // 16 * 16
        picture = torch.empty((status_at + 16 * B,), dtype=torch.uint8, device=self.device)
        status = picture[status_at:].view(torch.int32)

        def rows_and_pictures(model, p):
            """ the reader: the two draw launches go in front of the fetch of the rows they read, the pictures' copy behind it; after a
            range event the same again from the twin's rows, into the same buffer, over this call's frames """
            prims, prim_counts = hip.draw_build(p.pose_rows, P_d, score_threshold)
            hip.draw_raster(frames_d, raw_hw, Hr, Wr, prims, prim_counts, picture, status)
            poses, count = self.read_poses(model, p)
            return (poses, picture.cpu().numpy()), count

        poses, host = self._answer(plan, 'predict_composites_on_frames', rows_and_pictures)
        report = host[status_at:].view(np.int32).reshape(B, 4)
        if (report[:, 1] != 0).any():
            raise hip.GppError('gpp_draw_raster met {} records of an unknown kind'.format(int(report[:, 1].sum())))
        composites = [host[b * slot:b * slot + 2 * h * w * 3].reshape(2 * h, w, 3).copy() for b, (h, w) in enumerate(shapes)]
        return poses, scale, composites

    # Keras-style conveniences used by the reference's scripts
    def predict(self, inputs, batch_size=None, verbose=0):
        return self.predict_on_batch(inputs)

    def summary(self):
        print('{}: {} + FPN + heads, {} storage, {} conv launches'.format(
            self.name, self.backbone_name, self.dtype, len(self.conv_w)))
