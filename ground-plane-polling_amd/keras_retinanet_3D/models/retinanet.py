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
hand-written kernels of ../csrc; PyTorch only owns the device buffers.

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
import json
import os

import numpy as np

from ..backend import hip
from ..layers import conv as C
from ..layers import mobilenet as M
from ..layers.filter_detections import MAX_DETECTIONS, NMS_THRESHOLD, SCORE_THRESHOLD
from ..utils import anchors as anchor_utils
from ..utils import cuboid_nms as cuboid_nms_utils
from ..utils.gpp_utils import POLL_THRESHOLD, POSE_SCORE_THRESHOLD
from . import weights as W
# what a plan is (models/plan.py), under the names this module has always had: tests and tools spell them retinanet.StemDesc, retinanet.OP_CONV ...
from .plan import (BlockDesc, BlockProjDesc, FUSE_INPROJ_MIN_ROUNDS, CandidatePixelsDesc, DensePoolDesc, DetectDesc, PlanOp, PollDesc, PoolDesc, PoseDesc, CuboidNmsDesc,  # noqa: F401
                   PreactDesc, RaggedPoolDesc, RaggedStemDesc, ReluDesc, StemDesc, TailDesc,
                   OP_STEM, OP_MAXPOOL, OP_CONV, OP_RELU, OP_DETECT, OP_POLL, OP_TAIL, OP_BLOCK,
                   OP_DETECT_CANDIDATES, OP_DETECT_SELECT, OP_DETECT_EMIT, OP_DETECT_OSF, OP_STEM_POOL,
                   OP_MAXPOOL_PAD, OP_AVGPOOL, OP_CONV_PREACT, OP_MOBILENET_STEM, OP_MOBILENET_BLOCK, OP_POSE, OP_CUBOID_NMS,
                   OP_ABSMAX, OP_ABSMAX_CLEAR, OP_STEM_RAGGED, OP_STEM_POOL_RAGGED, OP_MAXPOOL_RAGGED,
                   OP_DETECT_CANDIDATE_PIXELS, DETECT_OPS, OP_JOIN, OP_SYNC,
                   PlanOptions, block_form, part_of, TOWER_SLICES, RANGE_AUDIT_THRESHOLD, X3_QUANTUM,
                   SPARSE_HEADS_MAX_SHARE, SPARSE_TOWER_MAX_SHARE, SPARSE_TOWER_MIN_ROUNDS, SPARSE_TOWER_DEPTH,
                   SPARSE_TOWER_DEEP_MAX_SHARE, SPARSE_TOWER_DEEP_MIN_ROUNDS, COMPUTE_UNITS, audit_report, SparseHeads, Plan)


class RetinaNet3D(object):
    """ Inference model: ResNet-50/101/152, DenseNet-121/169/201 or MobileNet (v1) + FPN + heads + decode + ground-plane polling. """

    def __init__(self, weights, backbone_name='resnet50', dtype='f16x3', nms=True, class_specific_filter=True,
                 orientation_specific_filter=False, name='retinanet-bbox', on_range_event=None, plan=None, pose=False, range_audit=False,
                 cuboid_nms=None):
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
        self._tuned = {}             # (layer, B, H, W) -> (tile_hint, split_k, us): see _autotune
        self.stem_x3 = False         # conv1 on the matrix pipe, input and weights split into two IEEE halves (_upload)
        self._load_tune_cache()
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
    def _anchor_table(self, hw, shapes=None):
        key = hw if shapes is None else (hw, tuple(shapes))
        if key not in self._anchors:
            a = anchor_utils.anchors_for_image(hw) if shapes is None else anchor_utils.anchors_for_shapes(shapes)
            self._anchors[key] = self.torch.as_tensor(a).to(self.device).contiguous()
        return self._anchors[key]

    def _desc(self, plan, name, inputs, outputs, K, stride=1, pad=None, relu=False, residuals=None, out_f32=False, lane=0):
        wt, bias, shape = self.conv_w[name]
        kh, kw, cin, cout = shape
        if pad is None:
            pad = (0, 0)
        # plan='latency': an explicit split-K factor per layer (a function of the layer alone); 0 = the library's own rule
        split = C.latency_split(kh, kw, cin, cout, sum(f.H * f.W for f in outputs)) if self.plan_mode == 'latency' else 0
        d = C.conv_desc(inputs, outputs, wt, bias, kh, kw, cin, cout, stride=stride, pad=pad, relu=relu,
                        residuals=residuals, dtype=self.dtype, out_f32=out_f32, out_scale=self.conv_scale.get(name), split_k=split)
        if self.dtype == 'f16x3':         # this plan's own range-event slot (Plan.range_slot): what its launches count no other plan sees
            d.range_counter = plan.range_slot.data_ptr()
        # split-K partial tiles: the workspace of this op's stream lane is allocated once every op is known (_build)
        plan.conv_descs.append((d, lane))
        plan.ws_need[lane] = max(plan.ws_need.get(lane, 0), C.workspace_bytes(d))
        return d

    def _conv(self, plan, name, inputs, outputs, K, stride=1, pad=None, relu=False, residuals=None, out_f32=False, tag=0, lane=0,
              join=False, sync=False):
        d = self._desc(plan, name, inputs, outputs, K, stride, pad, relu, residuals, out_f32, lane)
        plan.emit(OP_CONV, d, name, list(inputs) + list(residuals or []), outputs, tag=tag, flops=C.conv_flops(d), lane=lane, join=join,
                  sync=sync, io=(inputs, outputs, residuals))

    def _tail(self, plan, nm, a, y, shortcut, join=False, lane=0):
        """ branch2b (3x3) + branch2c (1x1, + shortcut, ReLU) of one bottleneck as ONE launch
        (gpp_bottleneck_tail): the intermediate map never reaches HBM.  Bit-identical to the two layers. """
        d1 = self._desc(plan, 'res{}_branch2b'.format(nm), [a], [a], 3, pad=(1, 1), relu=True)       # its `out` is never written
        d2 = self._desc(plan, 'res{}_branch2c'.format(nm), [a], [y], 1, relu=True, residuals=[shortcut])
        plan.emit(OP_TAIL, TailDesc(ctypes.addressof(d1), ctypes.addressof(d2), 0, 0), 'res{}_branch2b+2c'.format(nm), [a, shortcut], [y],
                  flops=C.conv_flops(d1) + C.conv_flops(d2), join=join, lane=lane, io=([a], [y], [shortcut]), inner=(d1, d2))

    def _block(self, plan, nm, x, a, bmap, y, shortcut, stride=1, join=False, lane=0):
        """ a whole bottleneck -- branch2a, branch2b, branch2c (+ shortcut, ReLU) -- as ONE launch (gpp_bottleneck_block): neither intermediate map
        reaches HBM (`a` / `bmap` only lend the descriptors their shapes).  Bit-identical to the three layers. """
        d1 = self._desc(plan, 'res{}_branch2a'.format(nm), [x], [a], 1, stride=stride, relu=True)
        d2 = self._desc(plan, 'res{}_branch2b'.format(nm), [a], [bmap], 3, pad=(1, 1), relu=True)
        d3 = self._desc(plan, 'res{}_branch2c'.format(nm), [bmap], [y], 1, relu=True, residuals=[shortcut])
        t = BlockDesc(ctypes.addressof(d1), ctypes.addressof(d2), ctypes.addressof(d3), 0, 0)
        plan.emit(OP_BLOCK, t, 'res{}_branch2a+2b+2c'.format(nm), [x, shortcut], [y], flops=C.conv_flops(d1) + C.conv_flops(d2) + C.conv_flops(d3),
                  join=join, lane=lane, io=([x], [y], [shortcut]), inner=(d1, d2, d3))

    def _block_proj(self, plan, nm, x, a, bmap, sc, y, join=False, lane=0):
        """ a whole projection bottleneck -- branch2a, branch1, branch2b, branch2c (+ shortcut, ReLU) -- as ONE launch (gpp_bottleneck_block_proj): the
        shortcut is computed from the input rows branch2a stages and never becomes a map (`a` / `bmap` / `sc` only lend the descriptors their
        shapes).  Bit-identical to the four layers. """
        d1 = self._desc(plan, 'res{}_branch2a'.format(nm), [x], [a], 1, relu=True)
        d2 = self._desc(plan, 'res{}_branch2b'.format(nm), [a], [bmap], 3, pad=(1, 1), relu=True)
        d3 = self._desc(plan, 'res{}_branch2c'.format(nm), [bmap], [y], 1, relu=True)
        dp = self._desc(plan, 'res{}_branch1'.format(nm), [x], [sc], 1)
        t = BlockProjDesc(ctypes.addressof(d1), ctypes.addressof(d2), ctypes.addressof(d3), 0, 1, ctypes.addressof(dp))
        plan.emit(OP_BLOCK, t, 'res{}_branch2a+2b+2c'.format(nm), [x], [y],
                  flops=C.conv_flops(d1) + C.conv_flops(d2) + C.conv_flops(d3) + C.conv_flops(dp), join=join, lane=lane, io=([x], [y], None),
                  inner=(d1, d2, d3, dp))

    def _preact(self, plan, name, inputs, outputs, relu=False):
        """ a 1x1 conv behind its input's BatchNormalization + ReLU (gpp_conv2d_preact): DenseNet's _1_conv and transition convs """
        d = self._desc(plan, name, inputs, outputs, 1, relu=relu)
        s, t = self.preact[name]
        plan.emit(OP_CONV_PREACT, PreactDesc(ctypes.addressof(d), s.data_ptr(), t.data_ptr()), name, inputs, outputs, flops=C.conv_flops(d),
                  io=(inputs, outputs, None), inner=(d,))

    def _stem(self, plan, opts, B, H, Wd, fmap, x):
        """ conv1 + bn + relu (7x7 / 2) and pool1 (3x3 / 2) into x.  opts.fuse_stem_pool: one launch, the (B, H1, W1, 64) conv map is never
        stored (bit-identical to the two launches: tests/test_stem_gpu.py; 16-bit types since round 2, the x3 types since round 6 --
        gpp_stem_pool_fused_x3: the float32 conv map was 274 MB written + read back at B = 8).  Else the conv map is stored and pooled by a
        second launch: ResNet's max pool, or DenseNet's zero-padded one into the channel prefix of its first concatenation buffer. """
        H1, W1 = (H + 6 - 7) // 2 + 1, (Wd + 6 - 7) // 2 + 1
        conv = x if opts.fuse_stem_pool else fmap(H1, W1, 64)
        d = StemDesc(plan.images.data_ptr(), self.stem_w.data_ptr(), self.stem_b.data_ptr(), conv.buf.data_ptr(),
                     hip.GPP_F16X3 if self.stem_x3 else C.gpp_storage_dtype(self.dtype), B, H, Wd,
                     plan.range_slot.data_ptr() if self.dtype == 'f16x3' else None)
        flops = 2.0 * B * H1 * W1 * 147 * 64
        plan.stem_out, plan.pool_out = (None if opts.fuse_stem_pool else conv), x
        if plan.ragged:
            # a batch of one height class: H = the 4 Hp rows of the canvas, H1 = 2 Hp the rows of the class's largest conv map; every image's own
            # height comes from plan.heights on the device (the same launches, per-image H / Ho / pad_top: csrc/stem_kernels.h)
            rd = RaggedStemDesc(d, plan.heights.data_ptr(), x.H, 0)
            if opts.fuse_stem_pool:
                plan.emit(OP_STEM_POOL_RAGGED, rd, 'conv1+pool1', [plan.images, plan.heights], [x], flops=flops)
                return
            plan.emit(OP_STEM_RAGGED, rd, 'conv1', [plan.images, plan.heights], [conv], flops=flops)
            pd = RaggedPoolDesc(PoolDesc(conv.buf.data_ptr(), x.buf.data_ptr(), C.gpp_storage_dtype(self.dtype), B, H1, W1, 64, 0),
                                plan.heights.data_ptr(), x.H, 0)
            plan.emit(OP_MAXPOOL_RAGGED, pd, 'pool1', [conv, plan.heights], [C.FMap(x.buf, B, x.H, x.W, 64, pitch=x.pitch)])
            return
        if opts.fuse_stem_pool:
            plan.emit(OP_STEM_POOL, d, 'conv1+pool1', [plan.images], [x], flops=flops)
            return
        plan.emit(OP_STEM, d, 'conv1', [plan.images], [conv], flops=flops)
        pooled = C.FMap(x.buf, B, x.H, x.W, 64, pitch=x.pitch)
        if self.densenet:
            pd = DensePoolDesc(conv.buf.data_ptr(), x.buf.data_ptr(), B, H1, W1, 64, 1, x.pitch)
            plan.emit(OP_MAXPOOL_PAD, pd, 'pool1', [conv], [pooled])
        else:
            pd = PoolDesc(conv.buf.data_ptr(), x.buf.data_ptr(), C.gpp_storage_dtype(self.dtype), B, H1, W1, 64, 0)
            plan.emit(OP_MAXPOOL, pd, 'pool1', [conv], [pooled])

    def _resnet_backbone(self, plan, opts, B, H, Wd, fmap, bmap):
        """ conv1 .. res5 of keras_resnet (bottleneck_2d: stride on the first 1x1) -> [C2, C3, C4, C5].  A stage runs as two half
        batches (opts.half_stages), the second half on side lane 1 beside the first, or chunk of images by chunk of images
        (opts.stage_chunks), one chunk after the other; the halves stay apart until the next whole-batch launch joins them. """
        H1, W1 = (H + 6 - 7) // 2 + 1, (Wd + 6 - 7) // 2 + 1
        x = fmap((H1 + 1) // 2, (W1 + 1) // 2, 64)
        self._stem(plan, opts, B, H, Wd, fmap, x)
        feats = []
        for stage, n_blocks in enumerate(W.BLOCKS[self.backbone_name]):
            f, xin, blocks = 64 * 2 ** stage, x, []
            for block in range(n_blocks):
                stride = 2 if (block == 0 and stage > 0) else 1
                ho, wo = (x.H - 1) // stride + 1, (x.W - 1) // stride + 1
                # (fused tails have no branch2b map: a fused block's descriptors borrow branch2a's -- neither is written)
                a, b = bmap(ho, wo, f), None if f in opts.fuse_tail else bmap(ho, wo, f)
                sc = bmap(ho, wo, 4 * f) if block == 0 else None
                x = bmap(ho, wo, 4 * f)
                blocks.append((W.block_name(self.backbone_name, stage, block), stride, a, b, sc, x))
            chunk = opts.stage_chunks[stage]
            halves = stage in opts.half_stages and chunk >= B       # (a stage that is chunked runs its chunks one after the other)
            parts = [(B // 2, B - B // 2, 1), (0, B // 2, 0)] if halves else [(c0, min(chunk, B - c0), 0) for c0 in range(0, B, chunk)]
            xs_of = {c0: part_of(xin, c0, nb) for c0, nb, _ in parts}
            for (nm, stride, a, b, sc, y), (c0, nb, lane) in ([(k, p) for k in blocks for p in parts] if halves else
                                                              [(k, p) for p in parts for k in blocks]):
                xs = xs_of[c0]
                join = not halves and bool(plan.open_lanes)          # the first launch of a whole-batch stage behind a split one
                form = block_form(opts, f, sc is not None, xs.split, halves, join, inproj=(stride, nb, y.H, y.W))
                xs_of[c0] = part_of(y, c0, nb)
                self._bottleneck(plan, nm, form, stride, xs, part_of(a, c0, nb), b and part_of(b, c0, nb),
                                 part_of(sc, c0, nb) if sc else xs, xs_of[c0], lane, join)
            feats.append(x)
        return feats

    def _bottleneck(self, plan, nm, form, stride, x, a, b, sc, y, lane, join):
        """ one bottleneck (of one batch part) in the form block_form chose.  join: its first launch closes the side lanes of the stage
        before; a projection shortcut on side lane 1 is joined by the launch that adds it. """
        launch, shortcut = form
        branch1 = 'res{}_branch1'.format(nm)
        if shortcut == 'inproj':
            self._block_proj(plan, nm, x, a, b or a, sc, y, join=join, lane=lane)
            return
        if shortcut == 'side':
            self._conv(plan, branch1, [x], [sc], 1, stride=stride, lane=1)
        if launch == 'block':
            if shortcut == 'inline':         # a projection block: the shortcut map first, in line, then the whole block
                self._conv(plan, branch1, [x], [sc], 1, stride=stride, lane=lane, join=join)
                join = False
            self._block(plan, nm, x, a, b or a, y, sc, stride=stride, join=join or shortcut == 'side', lane=lane)
            return
        self._conv(plan, 'res{}_branch2a'.format(nm), [x], [a], 1, stride=stride, relu=True, lane=lane, join=join)
        if shortcut == 'inline':
            self._conv(plan, branch1, [x], [sc], 1, stride=stride, lane=lane)
        if launch == 'tail':
            self._tail(plan, nm, a, y, sc, join=shortcut == 'side', lane=lane)
        else:
            self._conv(plan, 'res{}_branch2b'.format(nm), [a], [b], 3, pad=(1, 1), relu=True, lane=lane)
            self._conv(plan, 'res{}_branch2c'.format(nm), [b], [y], 1, relu=True, residuals=[sc], join=shortcut == 'side', lane=lane)

    def _densenet_backbone(self, plan, opts, B, H, Wd, fmap, bmap):
        """ conv1 .. conv5_block{N}_concat of keras' DenseNet (reference models/densenet.py:62-94) -> the four block concatenations.
        One float32 buffer per dense block at its final width: the block input (pool1 / the transition's average pool) is written into
        channels [0, C0), layer I's 32 channels into [C0 + 32 (I - 1), C0 + 32 I), and layer I's _1_conv reads the prefix [0, C0 + 32 (I - 1))
        through in_pitch.  The 128-channel map between _1_conv and _2_conv is pre-split for the x3 types.  The whole batch on lane 0. """
        widths = W.densenet_widths(self.backbone_name)
        H1, W1 = (H + 6 - 7) // 2 + 1, (Wd + 6 - 7) // 2 + 1
        h, w = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        cats = []
        for stage in range(4):
            cats.append(fmap(h, w, widths[stage]))
            h, w = h // 2, w // 2
        self._stem(plan, opts, B, H, Wd, fmap, cats[0])
        c0 = 64
        for stage, n in enumerate(W.DENSENET_BLOCKS[self.backbone_name]):
            cat = cats[stage]
            for i in range(1, n + 1):
                nm = 'conv{}_block{}'.format(stage + 2, i)
                cin = c0 + W.DENSENET_GROWTH * (i - 1)
                mid = bmap(cat.H, cat.W, W.DENSENET_BOTTLENECK)
                self._preact(plan, nm + '_1_conv', [C.FMap(cat.buf, B, cat.H, cat.W, cin, pitch=cat.pitch)], [mid], relu=True)
                self._conv(plan, nm + '_2_conv', [mid], [C.FMap(cat.buf, B, cat.H, cat.W, W.DENSENET_GROWTH, off=cin, pitch=cat.pitch)], 3,
                           pad=(1, 1))
            if stage == 3:
                break
            nm = 'pool{}'.format(stage + 2)
            t = fmap(cat.H, cat.W, widths[stage] // 2)
            self._preact(plan, nm + '_conv', [cat], [t])
            nxt = cats[stage + 1]
            pd = DensePoolDesc(t.buf.data_ptr(), nxt.buf.data_ptr(), B, t.H, t.W, t.C, 0, nxt.pitch)
            plan.emit(OP_AVGPOOL, pd, nm + '_pool', [t], [C.FMap(nxt.buf, B, nxt.H, nxt.W, t.C, pitch=nxt.pitch)])
            c0 = t.C
        return cats

    def _mobilenet_backbone(self, plan, opts, B, H, Wd, fmap, bmap):
        """ conv1 .. conv_pw_13_relu of keras' MobileNet (reference models/mobilenet.py:94-111) -> conv_pw_3 / 5 / 11 / 13 behind their
        ReLU6 (C2 .. C5).  conv1 is one launch (gpp_mobilenet_stem), every depthwise-separable block ONE launch (gpp_mobilenet_block: the
        depthwise map never reaches HBM).  Every map is float32, never pre-split; the whole batch on lane 0. """
        c0 = W.mobilenet_filters(self.backbone_name)[0]
        x = fmap(M.out_size(H, 2), M.out_size(Wd, 2), c0)
        sd = hip.MobileNetStemDesc(plan.images.data_ptr(), self.stem_w.data_ptr(), self.stem_b.data_ptr(), x.buf.data_ptr(), B, H, Wd, c0, x.pitch, 0)
        plan.stem_out, plan.pool_out = x, None
        plan.emit(OP_MOBILENET_STEM, sd, 'conv1', [plan.images], [x], flops=2.0 * B * x.H * x.W * 27 * c0)
        feats = []
        for i, cin, cout, stride in W.mobilenet_blocks(self.backbone_name):
            y = fmap(M.out_size(x.H, stride), M.out_size(x.W, stride), cout)
            dw_w, dw_b, pw_w, pw_b, scale = self.mbn_w[i]
            d = M.block_desc(x, y, dw_w, dw_b, pw_w, pw_b, scale, stride, self.dtype)
            plan.emit(OP_MOBILENET_BLOCK, d, 'conv_pw_{}'.format(i), [x], [y], flops=M.block_flops(d), io=([x], [y], None))
            x = y
            if i in W.MOBILENET_TAPS:
                feats.append(x)
        return feats

    def _pyramid(self, plan, opts, B, H, Wd, C3, C4, C5):
        """ the layout of every FPN / head tensor: the five levels back to back per image, (B, sum(H_l*W_l), C), so that one grouped
        launch covers all levels; a DenseNet's pyramid has the sizes of its own C3 .. C5 (floor pools).
        Returns (level shapes, pyramid(c, dtype=None) -> (buffer, its five level FMaps)). """
        got = [(C3.H, C3.W), (C4.H, C4.W), (C5.H, C5.W)]
        shapes = anchor_utils.pyramid_shapes_of_features(got) if self.densenet else anchor_utils.pyramid_shapes((H, Wd))
        if got != [tuple(s) for s in shapes[:3]]:
            raise RuntimeError('backbone / pyramid shape mismatch: {} vs {}'.format(got, shapes))
        pix = [h * w for h, w in shapes]
        total = sum(pix)
        plan.n_anchors = total * anchor_utils.NUM_BASE_ANCHORS
        x3s = opts.x3_level >= 1

        def pyramid(c, dtype=None):
            buf = self.torch.empty((B, total, c), dtype=dtype or self.tdtype, device=self.device)
            plan.keep.append(buf)
            sp = x3s and dtype is None
            return buf, [C.FMap(buf, B, h, w, c, off=sum(pix[:i]) * c, bstride=total * c, split=sp, half=self.dtype if sp else 'bf16x3')
                         for i, (h, w) in enumerate(shapes)]
        return shapes, pyramid

    def _fpn(self, plan, opts, C3, C4, C5, pyramid, smap):
        """ P3 .. P7 into one pyramid tensor (512 channels); returns its five level maps.  P5 and the P6 -> ReLU -> P7 chain are small
        launches (a few dozen tiles) independent of the C4 / C3 chain: with opts.fpn_lanes they run on the side streams underneath the
        C4_reduced / P4 launches (182 workgroups each: 74 CUs idle), joined by the fused first tower layer (measured +0.8 % on the f16x3
        step).  P4 (182 workgroups of 192 x 256: 71 % of the CUs) only feeds the towers: with opts.p4_lane it runs behind P5 on its side
        stream (re-forked: it needs T4), beside C3_reduced / P3. """
        _, P = pyramid(512)
        l_p5, l_p6 = (1, 2) if opts.fpn_lanes else (0, 0)
        T5 = smap(C5.H, C5.W, 512)
        self._conv(plan, 'C5_reduced', [C5], [T5], 1, join=bool(plan.open_lanes))
        self._conv(plan, 'P5', [T5], [P[2]], 3, pad=(1, 1), lane=l_p5)
        self._conv(plan, 'P6', [C5], [P[3]], 3, stride=2, pad=(C.same_pad(C5.H, 3, 2)[1], C.same_pad(C5.W, 3, 2)[1]), lane=l_p6)
        R6 = smap(P[3].H, P[3].W, 512)
        relu_d = ReluDesc(P[3].buf.data_ptr() + P[3].off * self.esz, R6.buf.data_ptr(), P[3].bstride, R6.bstride, P[3].H * P[3].W * 512,
                          C.gpp_dtype(self.dtype) if opts.x3_level >= 1 else C.gpp_storage_dtype(self.dtype), P[3].B)
        plan.emit(OP_RELU, relu_d, 'C6_relu', [P[3]], [R6], lane=l_p6)
        plan.relu_io = (P[3], R6)
        self._conv(plan, 'P7', [R6], [P[4]], 3, stride=2, pad=(C.same_pad(P[3].H, 3, 2)[1], C.same_pad(P[3].W, 3, 2)[1]), lane=l_p6)
        T4 = smap(C4.H, C4.W, 512)
        self._conv(plan, 'C4_reduced', [C4], [T4], 1, residuals=[T5])          # + UpsampleLike(P5, C4), fused
        self._conv(plan, 'P4', [T4], [P[1]], 3, pad=(1, 1), lane=opts.p4_lane, sync=bool(opts.p4_lane))
        T3 = smap(C3.H, C3.W, 512)
        self._conv(plan, 'C3_reduced', [C3], [T3], 1, residuals=[T4])          # + UpsampleLike(P4, C3), fused
        self._conv(plan, 'P3', [T3], [P[0]], 3, pad=(1, 1))
        return P

    def _detect(self, plan, B, anchors, pyramid):
        """ decode + NMS (RegressBoxes, RegressDims, FilterDetections): the three head outputs (float32 pyramids), the detection outputs,
        the workspace and the one descriptor the decode launches share, allocated before the towers are emitted.
        Returns ((classification, regression, dimension) output maps, decode(kind, name, **flags): records one decode launch). """
        torch, dev, D = self.torch, self.device, MAX_DETECTIONS
        f32, i32 = torch.float32, torch.int32
        plan.cls_logits, cls_o = pyramid(96, f32)
        plan.regression, reg_o = pyramid(144, f32)
        plan.regression_dim, dim_o = pyramid(36, f32)
        plan.boxes = torch.empty((B, D, 12), dtype=f32, device=dev)
        plan.dimensions = torch.empty((B, D, 3), dtype=f32, device=dev)
        plan.scores = torch.empty((B, D), dtype=f32, device=dev)
        plan.labels = torch.empty((B, D), dtype=i32, device=dev)
        plan.orientations = torch.empty((B, D), dtype=i32, device=dev)
        plan.anchor_index = torch.empty((B, D), dtype=i32, device=dev)
        plan.counts = torch.zeros((B,), dtype=i32, device=dev)
        need = hip.c_size_t(0)
        if self.osf and B > 16:
            raise ValueError('orientation_specific_filter=True handles at most 16 images per batch')
        size_fn = hip.lib().gpp_detect_osf_workspace_bytes if self.osf else hip.lib().gpp_detect_workspace_bytes
        hip.check(size_fn(B, plan.n_anchors, need), 'gpp_detect_workspace_bytes')
        plan.detect_ws = ws = torch.empty((int(need.value),), dtype=torch.uint8, device=dev)
        plan.anchors = anchors
        dd = DetectDesc(plan.cls_logits.data_ptr(), plan.regression.data_ptr(), plan.regression_dim.data_ptr(),
                        anchors.data_ptr(), plan.boxes.data_ptr(), plan.dimensions.data_ptr(), plan.scores.data_ptr(),
                        plan.labels.data_ptr(), plan.orientations.data_ptr(), plan.anchor_index.data_ptr(),
                        plan.counts.data_ptr(), ws.data_ptr(), ws.numel(), plan.n_anchors,
                        B, anchor_utils.NUM_BASE_ANCHORS, 1, D, SCORE_THRESHOLD, NMS_THRESHOLD if self.nms else 2.0)
        heads = [plan.cls_logits, plan.regression, plan.regression_dim]
        dets = [plan.boxes, plan.dimensions, plan.scores, plan.labels, plan.orientations, plan.anchor_index]
        access = {OP_DETECT_CANDIDATES: ([plan.cls_logits], [ws, plan.counts]), OP_DETECT_SELECT: ([ws, plan.regression], [ws]),
                  OP_DETECT_EMIT: (heads + [ws], dets)}

        def decode(kind, name='filtered_detections', **flags):
            reads, writes = access.get(kind, (heads, dets + [ws, plan.counts]))          # (OP_DETECT / OP_DETECT_OSF: the whole decode)
            if kind == OP_DETECT_CANDIDATE_PIXELS:      # the candidate pass + the pixel lists of the gathered head output layers, one op
                sp = plan.sparse
                lists = hip.PixelListDesc(ws.data_ptr(), sp.bitmap.data_ptr(), sp.rows.data_ptr(), sp.counts.data_ptr(), sp.flag.data_ptr(),
                                          plan.n_anchors, B, anchor_utils.NUM_BASE_ANCHORS, 4 if self.osf else 1, len(sp.level_pixels),
                                          sp.max_rows, 0, (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*sp.level_pixels), 0)
                if sp.tower_rows is not None:       # ... and their 3 x 3 dilation: what the regression tower's last layer has to write
                    lists.dilated_bitmap, lists.dilated_rows = sp.tower_bitmap.data_ptr(), sp.tower_rows.data_ptr()
                    lists.dilated_counts, lists.dilated_flag = sp.tower_counts.data_ptr(), sp.tower_flag.data_ptr()
                    lists.level_width = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*sp.level_widths)
                    lists.dilated_max_rows = sp.tower_max_rows
                reads, writes = access[OP_DETECT_CANDIDATES]
                plan.emit(kind, CandidatePixelsDesc(ctypes.addressof(dd), lists), name, reads, writes + sp.tensors(), inner=(dd,), **flags)
                return
            plan.emit(kind, dd, name, reads, writes, **flags)
        return (cls_o, reg_o, dim_o), decode

    def _heads(self, plan, opts, P, pyramid, outs, decode):
        """ the three towers (every layer one grouped launch over the five levels; layer 0 of the three shares its input: one fused
        launch, C_out = 896, whose channel slices layers 1..3 read) and the decode launches where their inputs are complete.
        opts.decode_overlap: classification, regression, dimension tower; the detection selection (one workgroup per image, 8 of the
        256 CUs) only needs the logits and the corner regressions, so it runs on a side stream underneath the dimension tower, and the
        decode of the <= 100 survivors joins when every head is done.  opts.head_lanes: the two small towers on side streams, filling
        the ramp-up / tail phases of the big regression-tower kernels.  opts.cls_lane: the classification tower (+ the candidate pass)
        on side lane 2 BESIDE the regression tower, whose last layer joins it. """
        cls_o, reg_o, dim_o = outs
        _, wide = pyramid(896)
        # (measured and rejected: the half-empty fourth 256-column tile of this 896-wide layer as its own 128-column launch
        # on a side stream -- the two launches do not pack into each other's partial rounds, no gain)
        self._conv(plan, 'pyramid_towers_0', P, wide, 3, pad=(1, 1), relu=True, join=True)

        def tower(prefix, width, c0, out_name, out, tag=0, lane=0, join=False):
            src = [C.FMap(m.buf, m.B, m.H, m.W, width, off=m.off + c0, bstride=m.bstride, pitch=m.pitch, split=m.split, half=m.half)
                   for m in wide]
            for i in range(1, 4):
                _, dst = pyramid(width)
                if i == 3 and out_name == 'pyramid_regression_ops' and plan.sparse is not None and plan.sparse.tower_rows is not None:
                    tower_last('{}_{}'.format(prefix, i), src, dst, tag, lane)
                elif out_name == 'pyramid_regression_ops' and plan.sparse is not None and 3 - plan.sparse.deep_layers <= i < 3:
                    tower_deep('{}_{}'.format(prefix, i), src, dst, tag, lane, 2 - i)
                else:
                    self._conv(plan, '{}_{}'.format(prefix, i), src, dst, 3, pad=(1, 1), relu=True, tag=tag, lane=lane)
                src = dst
            out_layer(out_name, src, out, lane, join)

        def tower_last(name, src, dst, tag, lane):
            """ the regression tower's last layer where its only reader is the gathered output layer (sparse_tower_form below): that launch
            reads the map at the listed pixels and their eight neighbours, so this layer has to write the 3 x 3 dilation of the lists and
            nothing else.  ONE op (its flops the algorithmic count, its tag the tower's): gpp_conv2d_igemm enqueues the dense launch and the
            gathered one on the dilated lists (gpp_conv_desc.tower_rows), and the lists' flag lets exactly one of them work -- the dense one
            whenever the output layer runs dense, which reads every row.  The op joins the candidates' lane: it is the first reader of the
            lists.  The rows nobody reads keep whatever the buffer held; Plan.complete_heads runs the layer dense before anyone reads more. """
            sp = plan.sparse
            d = self._desc(plan, name, src, dst, 3, pad=(1, 1), relu=True, lane=lane)
            d.tower_rows, d.tower_counts, d.tower_flag = sp.tower_rows.data_ptr(), sp.tower_counts.data_ptr(), sp.tower_flag.data_ptr()
            plan.emit(OP_CONV, d, name, list(src) + [sp.tower_rows, sp.tower_counts, sp.tower_flag], dst, tag=tag, flops=C.conv_flops(d), lane=lane,
                      join=not sp.lists_joined, io=(src, dst, None))
            sp.lists_joined = True
            sp.tower.append(d)

        def tower_deep(name, src, dst, tag, lane, which):
            """ layers 2 (which = 0) and 1 (which = 1) of the regression tower in a plan of the deep form (sparse_deep_layers below): the
            only reader of layer 2 is the gathered layer 3, which reads it on the 5 x 5 neighbourhoods of the candidates' pixels, and layer 1
            is read by the gathered layer 2 on the 7 x 7 ones.  ONE op each, as tower_last; the lists (gpp_conv_desc.deep_rows) come from
            gpp_detect_deep_lists behind pyramid_classification on this same stream, so there is no lane to join """
            sp = plan.sparse
            d = self._desc(plan, name, src, dst, 3, pad=(1, 1), relu=True, lane=lane)
            lists = [sp.deep_rows[which], sp.deep_counts[which], sp.deep_flags[which]]
            d.deep_rows, d.deep_counts, d.deep_flag = [t.data_ptr() for t in lists]
            plan.emit(OP_CONV, d, name, list(src) + lists, dst, tag=tag, flops=C.conv_flops(d), lane=lane, io=(src, dst, None))
            sp.deep.append(d)

        def sparse_deep_layers():
            """ how many tower layers in front of the last one take both forms (0, 1: layer 2, 2: layers 2 and 1) -- a rule of layer, map
            sizes, batch and plan options, like sparse_tower_form, which must hold: the lists are made on the caller's stream right behind
            pyramid_classification, so that layer runs there, unsplit, with the candidate pass on its side lane (decode_overlap without
            cls_lane: no head_lanes), in a plan that is neither orientation-specific nor an audit; and the dense launch of a layer fields more
            than opts.sparse_deep_rounds rounds of workgroups """
            if not opts.sparse_deep or opts.sparse_depth < 2 or not sparse_tower_form():
                return 0
            if opts.cls_lane or opts.head_lanes or self.osf or self.audit or not hasattr(hip.lib(), 'gpp_detect_deep_lists'):
                return 0
            rule = C.latency_split if self.plan_mode == 'latency' else C.default_split
            pixels = sum(f.H * f.W for f in reg_o)
            for name in ('pyramid_classification', 'pyramid_regression_1', 'pyramid_regression_2'):
                kh, kw, cin, cout = self.conv_w[name][2]
                if rule(kh, kw, cin, cout, pixels) > 1 or (name != 'pyramid_classification' and cout % 256):
                    return 0
            workgroups = sum((P[0].B * m.H * m.W + 255) // 256 for m in P) * (cout // 256)
            if not workgroups > opts.sparse_deep_rounds * COMPUTE_UNITS:
                return 0
            return min(2, opts.sparse_depth - 1)

        def sparse_tower_form():
            """ whether pyramid_regression_3 takes both forms: its reader pyramid_regression_ops is gathered in this plan (out_layer's own
            conditions), and the dense launch fields more than opts.sparse_tower_rounds rounds of 256 x 256 workgroups on the chip -- a rule
            of (layer, map sizes, batch) like the split rule: below one round a gathered launch costs one workgroup life either way """
            if not opts.sparse_heads or not opts.sparse_tower or not opts.decode_overlap or opts.x3_level < 1 or self.dtype not in C.X3_TYPES:
                return False
            kh, kw, cin, cout = self.conv_w['pyramid_regression_ops'][2]
            split = (C.latency_split if self.plan_mode == 'latency' else C.default_split)(kh, kw, cin, cout, sum(f.H * f.W for f in reg_o))
            kh, kw, cin, cout = self.conv_w['pyramid_regression_3'][2]
            split3 = (C.latency_split if self.plan_mode == 'latency' else C.default_split)(kh, kw, cin, cout, sum(f.H * f.W for f in reg_o))
            if split > 1 or split3 > 1 or cout % 256:
                return False
            workgroups = sum((P[0].B * m.H * m.W + 255) // 256 for m in P) * (cout // 256)
            return workgroups > opts.sparse_tower_rounds * COMPUTE_UNITS

        def out_layer(name, src, out, lane, join):
            """ the output layer of a tower.  opts.sparse_heads, regression and dimension tower: the decode reads these maps at candidate
            anchors only (nms_kernel, emit_kernel), and the candidate lists exist before the regression tower starts -- so the layer runs
            in gathered-row form on the pixels gpp_detect_pixel_lists listed (gpp_conv_desc.gather_rows: byte-identical rows, nothing else
            written).  The dense launch stays in the plan in front of it, guarded by the lists' flag: when more than max_rows rows are
            listed it runs and the gathered one returns at once, otherwise all its workgroups return on the flag -- no host round trip
            either way.  The first of the pair joins the candidates' lane unless a join has followed the lists already.  A layer the
            split-K rule splits (small maps) keeps its dense launch alone: one gathered launch cannot reproduce that summation order. """
            sp = plan.sparse
            kh, kw, cin, cout = self.conv_w[name][2]
            pixels = sum(f.H * f.W for f in out)
            split = (C.latency_split if self.plan_mode == 'latency' else C.default_split)(kh, kw, cin, cout, pixels)
            if sp is not None and sp.deep_layers and name == 'pyramid_classification':
                # the layer that writes the logits: gpp_conv2d_igemm enqueues the deep lists behind its launch (gpp_conv_desc.lists_after) --
                # part of this op, on this stream, in front of the tower layers that read them
                d = self._desc(plan, name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane)
                d.lists_after = sp.register_deep(sp.deep_desc(plan.cls_logits, plan.n_anchors, anchor_utils.NUM_BASE_ANCHORS, SCORE_THRESHOLD))
                plan.emit(OP_CONV, d, name, list(src), list(out) + sp.deep_tensors(), flops=C.conv_flops(d), lane=lane, join=join,
                          io=(src, out, None))
                return
            if sp is None or name == 'pyramid_classification' or lane or split > 1:
                self._conv(plan, name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane, join=join)
                if sp is not None and join and not lane:
                    sp.lists_joined = True
                return
            dense = self._desc(plan, name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane)
            dense.guard, dense.guard_value = sp.flag.data_ptr(), 1
            plan.emit(OP_CONV, dense, name, list(src) + [sp.flag], out, flops=C.conv_flops(dense), lane=lane, join=join or not sp.lists_joined,
                      io=(src, out, None))
            sp.lists_joined = True
            rows = self._desc(plan, name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane)
            rows.gather_rows, rows.gather_counts, rows.split_k = sp.rows.data_ptr(), sp.counts.data_ptr(), 1
            rows.guard, rows.guard_value = sp.flag.data_ptr(), 0
            # (flops 0: Plan.flops stays the reference graph's algorithmic count, which the dense launch above carries)
            plan.emit(OP_CONV, rows, name, list(src) + [sp.rows, sp.counts, sp.flag], out, lane=lane, io=(src, out, None))
            sp.dense.append(dense)
            sp.gathered.append(rows)

        l_dim, l_cls = (1, 2) if opts.head_lanes else (0, 0)
        towers = {'cls': ('pyramid_classification', 256, 512, 'pyramid_classification', cls_o, 0, l_cls or opts.cls_lane),
                  'reg': ('pyramid_regression', 512, 0, 'pyramid_regression_ops', reg_o, 1, 0, bool(opts.cls_lane)),
                  'dim': ('pyramid_regression_dim', 128, 768, 'pyramid_regression_dim', dim_o, 0, l_dim)}
        if opts.sparse_heads:
            plan.sparse = SparseHeads(self.torch, self.device, P[0].B, [m.H * m.W for m in P], opts.sparse_heads, [m.W for m in P],
                                      opts.sparse_tower if sparse_tower_form() else 0.0)
            plan.keep += plan.sparse.tensors()
            layers = sparse_deep_layers()
            if layers:
                plan.sparse.add_deep(self.torch, layers, opts.sparse_deep)
                plan.keep += plan.sparse.deep_tensors()
        if opts.decode_overlap:
            tower(*towers['cls'])
            decode(OP_DETECT_CANDIDATE_PIXELS if plan.sparse else OP_DETECT_CANDIDATES, 'filtered_detections/candidates',
                   lane=opts.cls_lane or 1)     # on the tower's lane when it has one
            tower(*towers['reg'])
            decode(OP_DETECT_SELECT, 'filtered_detections/select', lane=1, sync=True)
            tower(*towers['dim'])
            decode(OP_DETECT_EMIT, join=True)
        else:
            for t in ('dim', 'cls', 'reg'):
                tower(*towers[t])
            decode(OP_DETECT_OSF if self.osf else OP_DETECT, join=True)

    def _poll(self, plan, B, n_planes, planes_batched):
        """ ground-plane polling (FitRoadPlanes) of the detections """
        torch, dev, D = self.torch, self.device, MAX_DETECTIONS
        plan.keypoints = torch.empty((B, D, 4, 3), dtype=torch.float32, device=dev)
        plan.keyplanes = torch.empty((B, D, 1, 4), dtype=torch.float32, device=dev)
        plan.residuals = torch.empty((B, D), dtype=torch.float32, device=dev)
        plan.best_index = torch.empty((B, D), dtype=torch.int32, device=dev)
        need = hip.c_size_t(0)
        hip.check(hip.lib().gpp_poll_workspace_bytes(B, n_planes, int(planes_batched), need), 'gpp_poll_workspace_bytes')
        plan.poll_ws = torch.empty((max(int(need.value), 16),), dtype=torch.uint8, device=dev)
        pd = PollDesc(plan.boxes.data_ptr(), plan.dimensions.data_ptr(), plan.orientations.data_ptr(), plan.P_inv.data_ptr(),
                      plan.planes.data_ptr(), plan.keypoints.data_ptr(), plan.keyplanes.data_ptr(), plan.residuals.data_ptr(),
                      plan.best_index.data_ptr(), plan.poll_ws.data_ptr(), plan.poll_ws.numel(), B, D, n_planes,
                      int(planes_batched), POLL_THRESHOLD, 0)
        plan.emit(OP_POLL, pd, 'fit_road_planes', [plan.boxes, plan.dimensions, plan.orientations, plan.P_inv, plan.planes],
                  [plan.keypoints, plan.keyplanes, plan.residuals, plan.best_index, plan.poll_ws], tag=2,    # tag 2: bench.py times it live too
                  flops=162.0 * B * D * n_planes)

    def _pose(self, plan, B):
        """ 6-DoF pose + KITTI fields of the detections (what bin/run_network.py does on the host after predict_on_batch), on lane 0
        behind the polling.  Rows, range-event snapshot and counts share ONE flat buffer, so that one copy brings a call's result to
        the host: [B x D x 36 rows | 2 words: the plan's range counter as the stream saw it | B counts (int32 bits)]. """
        torch, dev, D = self.torch, self.device, MAX_DETECTIONS
        n = B * D * hip.GPP_POSE_COLS
        plan.pose_out = torch.zeros((n + 2 + B,), dtype=torch.float32, device=dev)
        plan.pose_rows = plan.pose_out[:n].view(B, D, hip.GPP_POSE_COLS)
        plan.pose_counts = plan.pose_out[n + 2:].view(torch.int32)
        # per image: the image scale, the raw image's height and width (predict_poses_*: uploaded with P_inv; a captured graph reads
        # the buffer, not the values).  Until a caller says otherwise: the frame as it is, scale 1
        plan.frame_info = torch.tensor([[1.0, plan.shape[1], plan.shape[2]]] * B, dtype=torch.float32, device=dev)
        pd = PoseDesc(plan.boxes.data_ptr(), plan.dimensions.data_ptr(), plan.scores.data_ptr(), plan.labels.data_ptr(),
                      plan.orientations.data_ptr(), plan.keypoints.data_ptr(), plan.residuals.data_ptr(), plan.frame_info.data_ptr(),
                      plan.pose_rows.data_ptr(), plan.pose_counts.data_ptr(), B, D, POSE_SCORE_THRESHOLD, 0)
        plan.emit(OP_POSE, pd, 'recover_pose', [plan.boxes, plan.dimensions, plan.scores, plan.labels, plan.orientations, plan.keypoints,
                                                plan.residuals, plan.frame_info], [plan.pose_rows, plan.pose_counts])

    def _cuboid_nms(self, plan, B):
        """ cuboid_nms=(metric, threshold): the greedy NMS of the cuboids (gpp_cuboid_nms_f64) on lane 0 behind the pose op, in place on
        its rows and counts; plan.pose_suppressor (B, D) int32 names the kept row that removed each suppressed one """
        metric, threshold = self.cuboid_nms
        D = MAX_DETECTIONS
        plan.pose_suppressor = self.torch.full((B, D), -1, dtype=self.torch.int32, device=self.device)
        nd = CuboidNmsDesc(plan.pose_rows.data_ptr(), plan.pose_counts.data_ptr(), plan.pose_suppressor.data_ptr(), threshold, B, D,
                           cuboid_nms_utils.metric_code(metric), 0)
        plan.emit(OP_CUBOID_NMS, nd, 'suppress_cuboids', [plan.pose_rows], [plan.pose_rows, plan.pose_counts, plan.pose_suppressor])

    def _audit(self, plan):
        """ range_audit=True: one gpp_channel_absmax launch behind every launch that writes (a part, a level or a channel slice of) a map
        that some convolution of the plan reads as its activation operand or adds as its residual -- the maps an x3 loop splits into
        (hi, lo) halves or reads pre-split -- on that launch's lane, into the map's row of plan.audit_table; the first op of the plan
        clears the table on the stream.  A map is a channel range of a buffer as its READERS name it (the three towers read three
        slices of the fused first layer's 896 channels: three maps; the five levels of a pyramid tensor: one map).  Placed once every
        op is known: who reads what is only known then.  Operands that never exist in HBM go to plan.audit_unobserved. """
        torch, esz = self.torch, self.esz
        views, order = {}, []                       # (buffer, pitch, first channel, channels) -> record

        def key_of(f):
            return (f.buf.data_ptr(), f.pitch, f.off % f.pitch, f.C)

        for pos, (kind, _, desc, name, _) in enumerate(plan.ops):
            io = plan.op_io[pos]
            if kind == OP_CONV_PREACT:
                lo, hi = min(a for a, _ in Plan.spans(io[0])), max(b for _, b in Plan.spans(io[0]))
                plan.audit_unobserved.append({'name': name + '/operand', 'consumers': [name], 'extent': (lo, hi),
                                              'reason': 'max(x * scale + shift, 0) is formed after the load (gpp_conv2d_preact)'})
            elif kind == OP_MOBILENET_BLOCK:
                plan.audit_unobserved.append({'name': name.replace('conv_pw_', 'conv_dw_'), 'consumers': [name], 'extent': None,
                                              'reason': 'the depthwise result lives in LDS (gpp_mobilenet_block); bounded by ReLU6'})
            elif kind == OP_CONV:
                for f in list(io[0]) + list(io[2] or []):
                    k = key_of(f)
                    if k not in views:
                        views[k] = {'consumers': [], 'producers': [], 'channels': f.C, 'spans': [], 'fmaps': [], 'split': f.split,
                                    'layout': 'split_f16' if f.split else 'f32'}
                        order.append(k)
                    if name not in views[k]['consumers']:
                        views[k]['consumers'].append(name)
                    views[k]['spans'] += Plan.span(f)
                    if not any((g.off, g.B, g.H, g.W) == (f.off, f.B, f.H, f.W) for g in views[k]['fmaps']):
                        views[k]['fmaps'].append(f)
        offset = 0
        for k in order:
            views[k]['row'] = (offset, k[3])
            offset += k[3]
        plan.audit_table = table = torch.zeros((max(offset, 1),), dtype=torch.int32, device=self.device)       # (uint32 bit patterns)
        extra = {}
        for pos, (kind, _, desc, name, _) in enumerate(plan.ops):
            for k in order:
                ptr, pitch, c0, c = k
                outs = [o for o in plan.wrote[pos] if o.buf.data_ptr() == ptr and o.pitch == pitch]
                if not outs:
                    continue
                oc0, oc = outs[0].off % pitch, outs[0].C
                lo, hi = max(c0, oc0), min(c0 + c, oc0 + oc)
                if lo >= hi:
                    continue
                v = views[k]
                if name not in v['producers']:
                    v['producers'].append(name)
                # the pixels this launch wrote, as runs of consecutive pixels of the buffer (a dense batch, the five levels of every
                # image of a pyramid tensor: one run; one level of a pyramid tensor: one run per image)
                runs = []
                for start, n in sorted(((o.off - oc0 + b * o.bstride) // pitch, o.H * o.W) for o in outs for b in range(o.B)):
                    if runs and runs[-1][0] + runs[-1][1] == start:
                        runs[-1][1] += n
                    else:
                        runs.append([start, n])
                row = table[v['row'][0] + lo - c0:v['row'][0] + hi - c0]
                for start, n in runs:
                    d = hip.AbsmaxDesc(ptr + start * pitch * esz, row.data_ptr(), n, pitch, hi - lo, lo,
                                       hip.GPP_ABSMAX_SPLIT_F16 if v['split'] else hip.GPP_ABSMAX_F32, 0)
                    extra.setdefault(pos, []).append((OP_ABSMAX, d, 'absmax:' + name, outs, [row]))
        plan.insert_behind(extra)
        plan.keep.append(table)
        clear = hip.AbsmaxClearDesc(table.data_ptr(), table.numel())
        plan.emit(OP_ABSMAX_CLEAR, clear, 'absmax:clear', [], [table])
        for lst in (plan.ops, plan.lanes, plan.access, plan.atomic, plan.wrote, plan.op_io):       # ... as the FIRST op of the plan
            lst.insert(0, lst.pop())
        for k in order:
            v = views[k]
            names = v['producers']
            if not names:
                raise RuntimeError('range audit: no launch of the plan writes the operand of {}'.format(v['consumers']))
            # a channel slice of a launch's output carries the name of the layer it is in the reference (the fused first tower layer)
            name = TOWER_SLICES.get((names[0], k[2]), names[0]) if len(names) == 1 else \
                '+'.join(sorted(names)) if len(names) <= 5 else '{}..{}'.format(names[0], names[-1])
            plan.audit_maps.append({'name': name, 'producers': names, 'consumers': v['consumers'], 'channels': v['channels'],
                                    'layout': v['layout'], 'row': v['row'], 'fmaps': v['fmaps'],
                                    'extent': (min(a for a, _ in v['spans']), max(b for _, b in v['spans']))})

    def _bind_workspaces(self, plan):
        """ split-K partial tiles of the deep-K layers with a tiny per-image grid (res5 branch2b, P5..P7): one workspace per stream lane
        (concurrent launches must not share partial tiles), sized from the descriptors of the whole plan """
        plan.workspaces = {lane: self.torch.empty((max(need, 16),), dtype=self.torch.uint8, device=self.device)
                           for lane, need in plan.ws_need.items()}
        for d, lane in plan.conv_descs:
            d.partial = plan.workspaces[lane].data_ptr()
            d.partial_bytes = plan.workspaces[lane].numel()

    def _plan_options(self, B):
        """ every GPP_* switch of the plan builder, read once per plan (at the start of _build), as its effective value for this model
        and batch (PlanOptions) """
        env = os.environ.get
        x3 = self.dtype in C.X3_TYPES
        # x3 types: maps written and read by convolutions only are stored PRE-SPLIT ([32 hi | 32 lo] halves per 32 channels,
        # gpp_conv_desc.x3_split): GPP_X3_SPLIT=2 (default) every such map, 1 = only the maps between the FPN / head layers -- 80 % of the
        # FLOPs, all of them matrix-pipe bound -- 0 = none.  Written that way by the producing layer's epilogue, read by the consumers
        # without the per-fragment split on the vector ALU.
        x3_level = int(env('GPP_X3_SPLIT', '2')) if x3 else 0
        # GPP_STAGE_CHUNKS="2,4,8,8": a stage chunk of images by chunk of images, to keep a chunk's working set inside the 256 MiB Infinity
        # Cache; measured on MI355X at B = 8 this LOSES 1-6 % (the smaller launches cost more than the on-die re-reads save): off
        chunks = env('GPP_STAGE_CHUNKS')
        # GPP_FUSE_TAIL: widths whose branch2b + branch2c run as one launch ("" or 0 for none).  Measured at B = 8, same box, whole step:
        # none 1553, res3 only 1562, res2 + res3 1571 images/s (in isolation the fused res2 launch is no faster than its two layers --
        # 122 us vs 36 + 80 -- but the step is: 69 MB less through HBM per block).  The x3 form (bottleneck_tail_x3_kernel) reads
        # pre-split maps at C = 64 (res2) only -- at C = 128 its LDS footprint leaves one workgroup per CU; float32 operands: none
        fuse_tail = [int(v) for v in env('GPP_FUSE_TAIL', '64,128').split(',') if v.strip() and int(v) > 0]
        if x3:
            fuse_tail = [v for v in fuse_tail if v == 64] if x3_level >= 2 else []
        elif self.esz == 4:
            fuse_tail = []
        # GPP_FUSE_BLOCK: widths whose IDENTITY blocks (branch2a + 2b + 2c + shortcut) run as one launch (gpp_bottleneck_block; x3 types on
        # pre-split maps): res2 (C = 64: 4-wavefront workgroups, two per CU; x in once, y out once: 245 -> 212 us per block at B = 8) and
        # res3 (C = 128: 8 wavefronts, one per CU; at parity with its three launches in isolation, half their fabric bytes).  Same-box A/B
        # of the step (profiles/r6/ab_fuse_block_*.txt): B = 8: 780 -> 793 images/s (+1.7 %) with both, +0.9 % with res2 alone; B = 4
        # +1.2 %, B = 2 +0.7 %, batch-1 plan 2.67 -> 2.65 ms.  "" for the separate launches (bit-identical either way).  Projection
        # blocks too (GPP_FUSE_BLOCK_PROJ=1) measured -0.6 %: off.
        fuse_block = [int(v) for v in env('GPP_FUSE_BLOCK', '64,128').split(',') if v.strip()] if (x3 and x3_level >= 2) else []
        if self.audit:
            # an audit plan reads every operand map in HBM: the separate launches wherever a fused form keeps one in LDS (bit-identical
            # to them: tests/test_block_gpu.py), so the results do not change
            fuse_tail, fuse_block = [], []
        head_lanes = env('GPP_HEAD_LANES', '0') != '0'
        fpn_lanes = head_lanes or env('GPP_FPN_LANES', '1') != '0'
        overlap = env('GPP_DECODE_OVERLAP', '1') != '0' and not head_lanes and not self.osf
        return PlanOptions(
            x3_level=x3_level,
            fuse_stem_pool=not self.densenet and not self.mobilenet and (self.esz == 2 or self.stem_x3) and env('GPP_FUSE_STEM_POOL', '1') != '0',
            stage_chunks=tuple(max(1, min(B, int(v))) for v in chunks.split(',')) if chunks else (B,) * 4,
            # GPP_HALF_LANES (default "0,1,2,3" = res2 .. res5; "" for whole batches): a launch of these stages fills the 256 CUs 0.7 - 1.4
            # times and is bound by tile fills and first-touch latency; two half-batch chains in flight overlap one's prologue / epilogue /
            # barrier waits with the other's main loop (f16x3 step, same box: 775 -> 793 images/s; three parts: 801 against 811).  res2
            # since round 6, with fused identity blocks: B = 8 +0.7 %, B = 4 +1.1 %, B = 2 +1.1 % (profiles/r6/ab_half_lanes_with_blocks.txt)
            half_stages=frozenset(int(v) for v in env('GPP_HALF_LANES', '0,1,2,3').split(',') if v.strip()) if B >= 2 else frozenset(),
            fuse_tail=tuple(v for v in fuse_tail if v in (64, 128)),
            fuse_block=tuple(v for v in fuse_block if v in (64, 128)),
            fuse_block_proj=env('GPP_FUSE_BLOCK_PROJ', '0') != '0',
            # GPP_FUSE_BLOCK_INPROJ (default 1; with 64 in GPP_FUSE_BLOCK): res2a -- the stride-1 projection block -- as ONE launch that computes the
            # shortcut itself (gpp_bottleneck_block_proj): no res2a_branch1 launch, no shortcut map through HBM (276 MB written and read back at
            # B = 8).  Only where a batch part's launch fields more than GPP_FUSE_INPROJ_MIN_ROUNDS rounds of 2 x 256 workgroups of 8 x 14 pixels
            # (a rule of layer, map size and batch part); 0 = res2a as three launches.  Bit-identical either way.
            fuse_block_inproj=env('GPP_FUSE_BLOCK_INPROJ', '1') != '0',
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
            sparse_heads=(max(1e-9, float(env('GPP_SPARSE_HEADS_MAX_SHARE', SPARSE_HEADS_MAX_SHARE)))
                          if (overlap and not self.audit and env('GPP_SPARSE_HEADS', '1') != '0') else 0.0),
            # GPP_SPARSE_TOWER (default 1; with sparse head outputs only): the regression tower's LAST layer on the 3 x 3 dilation of the
            # candidates' pixels -- the only rows its reader, the gathered output layer, takes.  The value is the largest share of all
            # pyramid pixels the gathered launch takes (GPP_SPARSE_TOWER_MAX_SHARE); GPP_SPARSE_TOWER_MIN_ROUNDS: the rounds of workgroups
            # the dense launch must exceed (0 in tests: small plans take the form too)
            sparse_tower=(max(1e-9, float(env('GPP_SPARSE_TOWER_MAX_SHARE', SPARSE_TOWER_MAX_SHARE)))
                          if (overlap and not self.audit and env('GPP_SPARSE_HEADS', '1') != '0' and env('GPP_SPARSE_TOWER', '1') != '0') else 0.0),
            sparse_tower_rounds=float(env('GPP_SPARSE_TOWER_MIN_ROUNDS', SPARSE_TOWER_MIN_ROUNDS)),
            # GPP_SPARSE_TOWER_DEPTH (default 3; with the sparse tower only): how many layers of the regression tower run on the rows their
            # reader takes -- 1 the last layer alone, 2 layer 2 as well (the 5 x 5 dilation of the candidates' pixels), 3 layer 1 too (7 x 7).
            # The lists of layers 2 and 1 are made from the logits on the caller's stream (gpp_detect_deep_lists);
            # GPP_SPARSE_TOWER_DEEP_MAX_SHARE: the largest share of rows their gathered launches take; GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS: the
            # rounds of workgroups their dense launch must exceed (its own variable: tests force the tower's to 0 at small shapes)
            sparse_deep=max(1e-9, float(env('GPP_SPARSE_TOWER_DEEP_MAX_SHARE', SPARSE_TOWER_DEEP_MAX_SHARE))),
            sparse_deep_rounds=float(env('GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS', SPARSE_TOWER_DEEP_MIN_ROUNDS)),
            sparse_depth=int(env('GPP_SPARSE_TOWER_DEPTH', SPARSE_TOWER_DEPTH)),
            tune_key='x3split={};fuse={}/{};plan={}{}'.format(env('GPP_X3_SPLIT', '2'), env('GPP_FUSE_TAIL', '64,128'), env('GPP_FUSE_BLOCK', '64,128'),
                                                              self.plan_mode, C.latency_split_config() if self.plan_mode == 'latency' else '') +
                     (';audit' if self.audit else '') + ('' if env('GPP_FUSE_BLOCK_INPROJ', '1') != '0' else ';inproj=0'))      # (the default keeps its key)

    def _build(self, B, H, Wd, n_planes, planes_batched, ragged=False):
        """ ragged: the plan of a height class (utils/image.py) -- H = 4 Hp is the row count of the canvas, and the stem and pool1 take
        every image's own height from plan.heights (int32, on the device: data of the plan, so one plan and one captured graph serve
        every mix of heights); everything behind pool1 is the uniform plan's """
        torch, dev = self.torch, self.device
        if ragged:
            if self.mobilenet or self.densenet:
                raise ValueError('{} has no ragged form: {}; run its images grouped by shape'.format(
                    self.backbone_name, 'its first block runs at conv1\'s resolution, which differs inside a height class' if self.mobilenet
                    else 'its zero-padded pool1 (gpp_maxpool3x3s2_pad_f32) has no per-image form'))
            if self.audit:
                raise ValueError('range_audit=True has no ragged form: the audit of the conv1 map reads rows that a shorter image does not have')
            if H % 4:
                raise ValueError('the canvas of a ragged plan has 4 Hp rows, got {}'.format(H))
        opts = self._plan_options(B)
        plan = Plan()
        plan.shape = (B, H, Wd, n_planes, planes_batched)
        plan.ragged = bool(ragged)
        if ragged:
            plan.heights = torch.full((B,), H, dtype=torch.int32, device=dev)
            plan.heights_host = [H] * B
        plan.side_lanes = {'fpn': opts.fpn_lanes, 'branch1': opts.br1_lane, 'p4': bool(opts.p4_lane),
                           'half_batch_stages': sorted(opts.half_stages), 'cls_tower': bool(opts.cls_lane)}
        plan.decode_overlap = opts.decode_overlap
        # dtype='f16x3': the 8-byte counter every launch of THIS plan adds its range events to (gpp_conv_desc.range_counter, gpp_stem_desc.range_counter),
        # never reset by anyone but x3_range_events(reset=True) of this model; range_seen = its value when a result of the plan was last fetched
        plan.range_slot = torch.zeros((1,), dtype=torch.int64, device=dev)
        plan.range_seen = 0
        plan.images = torch.empty((B, H, Wd, 3), dtype=torch.float32, device=dev)
        plan.P_inv = torch.empty((B, 4, 3), dtype=torch.float32, device=dev)
        plan.planes = torch.empty((B, n_planes, 4) if planes_batched else (n_planes, 4), dtype=torch.float32, device=dev)

        def fmap(h, w, c, split=False):
            f = C.FMap.empty(B, h, w, c, self.tdtype, dev, half=self.dtype if self.dtype in C.X3_TYPES else 'bf16x3')
            plan.keep.append(f.buf)
            return f.mark_split() if split else f

        backbone = self._densenet_backbone if self.densenet else self._mobilenet_backbone if self.mobilenet else self._resnet_backbone
        C2, C3, C4, C5 = backbone(plan, opts, B, H, Wd, fmap, lambda h, w, c: fmap(h, w, c, opts.x3_level >= 2))
        plan.features = {'stem': plan.stem_out, 'C2': C2, 'C3': C3, 'C4': C4, 'C5': C5}
        shapes, pyramid = self._pyramid(plan, opts, B, H, Wd, C3, C4, C5)
        P = self._fpn(plan, opts, C3, C4, C5, pyramid, lambda h, w, c: fmap(h, w, c, opts.x3_level >= 1))
        plan.features.update({'P{}'.format(i + 3): P[i] for i in range(5)})
        outs, decode = self._detect(plan, B, self._anchor_table((H, Wd), shapes if self.densenet else None), pyramid)
        self._heads(plan, opts, P, pyramid, outs, decode)
        self._poll(plan, B, n_planes, planes_batched)
        if self.pose:
            self._pose(plan, B)
        if self.cuboid_nms is not None:
            self._cuboid_nms(plan, B)
        if self.audit:
            self._audit(plan)
        self._bind_workspaces(plan)
        plan.finalize()
        plan.tagged = [name for _, tag, _, name, _ in plan.ops if tag]
        if opts.autotune:
            self._autotune(plan)
        return plan

    # ------------------------------------------------------------------ per-layer tile selection
    def _tune_cache_path(self):
        return os.environ.get('GPP_TUNE_CACHE')

    def _tune_config(self):
        """ what a cached tile choice is valid for besides (backbone, type, layer, batch, image size): the build of the library (tile codes
        come and go with it: gpp_version() carries a hash of the kernel sources) and the plan options that change which maps are
        pre-split or fused (PlanOptions.tune_key, the same at every batch) -- a tile timed on a float32 map may not even exist for the
        pre-split form of the same layer """
        ver = hip.lib().gpp_version().decode().split('src:')[-1]
        return 'v2;{};{}'.format(ver, self._plan_options(1).tune_key)

    def _load_tune_cache(self):
        path = self._tune_cache_path()
        if path and os.path.exists(path):
            with open(path) as f:
                for key, val in json.load(f).items():
                    parts = key.split('|')
                    if len(parts) != 7:              # (files of rounds 1-3: no library hash in the key -- ignored, the layers are timed again)
                        continue
                    cfg, bb, dt, name, b, h, w = parts
                    if cfg == self._tune_config() and bb == self.backbone_name and dt == self.dtype:
                        self._tuned[(name, int(b), int(h), int(w))] = (int(val[0]), float(val[-1]))

    def _save_tune_cache(self):
        """ Rank 0 only, through a temporary file + os.replace: readers never see a torn file, ranks never race. """
        path = self._tune_cache_path()
        if not path or int(os.environ.get('RANK', '0')) != 0:
            return
        data = {}
        if os.path.exists(path):
            try:
                with open(path) as f:
                    data = json.load(f)
            except ValueError:
                data = {}
        for (name, b, h, w), val in self._tuned.items():
            data['|'.join([self._tune_config(), self.backbone_name, self.dtype, name, str(b), str(h), str(w)])] = list(val)
        tmp = '{}.tmp.{}'.format(path, os.getpid())
        with open(tmp, 'w') as f:
            json.dump(data, f, indent=0, sort_keys=True)
        os.replace(tmp, path)

    def _autotune(self, plan):
        """ Choose the block tile of every conv layer of this plan by timing the candidates on the device
        (gpp_conv2d_autotune), layer by layer on realistic activations (a noise frame pushed through the layers
        before).  Whether a layer's tile grid fills the 256 CUs in 1.07 or 0.95 rounds decides its time by up to 1.5x
        and is cheap to measure.  The tile NEVER changes a result (same K order per output element,
        test_every_tile_gives_identical_results), so ranks and plans may choose differently without any effect on the
        outputs; split-K, which would, is not tuned (gpp_conv2d_split_rule).  Choices are remembered per (layer, batch,
        image size) and can be persisted with GPP_TUNE_CACHE=<file.json>.  GPP_AUTOTUNE=0 keeps the library heuristic.
        The fused tails choose their row count (tile_rows), DenseNet's pre-activation convs the tile of their inner conv, MobileNet's
        blocks their own tile_hint. """
        self._require_hip()
        H, Wd = plan.shape[1:3]
        plan.images.uniform_(-120.0, 130.0)
        fresh = False
        plan.tuning = {}
        # GPP_TUNE_RANDOM=<seed> (tests / tools/first_run_stress.py): every layer takes a RANDOM tile among those the library
        # accepts for it instead of the fastest one -- the outputs may not change by a bit, whatever the draw
        rnd = None
        if os.environ.get('GPP_TUNE_RANDOM'):
            import random
            rnd = random.Random(int(os.environ['GPP_TUNE_RANDOM']) * 1000003 + int(os.environ.get('RANK', '0')))
        for index, (kind, _, desc, name, flops) in enumerate(plan.ops):
            if kind in DETECT_OPS or kind == OP_POLL:
                continue
            gathered = kind == OP_CONV and bool(desc.gather_rows)
            if kind == OP_CONV and desc.guard:
                # a guarded pair of the sparse head outputs: the dense launch is timed with the flag set, the gathered one with the flag
                # clear on a synthetic list of every 8th pixel (a run's own lists do not exist yet: the decode ops are not run here)
                plan.sparse.flag.fill_(0 if gathered else 1)
                if gathered:
                    plan.sparse.put_every_nth(self.torch)
                    name = name + '@rows'
            self.run_op(plan, index)
            if kind not in (OP_CONV, OP_TAIL, OP_CONV_PREACT, OP_MOBILENET_BLOCK):
                continue
            # where the choice is written: the conv's own descriptor, the pre-activation's inner one, the tail's row count
            target = plan.inner[id(desc)][0] if kind == OP_CONV_PREACT else desc
            field = 'tile_rows' if kind == OP_TAIL else 'tile_hint'
            if rnd is not None:
                setattr(target, field, rnd.choice(self._tile_choices(plan, index, kind, target)))
                plan.tuning[name] = (int(getattr(target, field)), 0.0)
                self.run_op(plan, index)
                continue
            key = (name, target.B if kind == OP_MOBILENET_BLOCK else (plan.inner[id(desc)][0] if kind == OP_TAIL else target).batch, H, Wd)     # (a half-batch launch is tuned as what it is)
            if kind == OP_CONV and key in self._tuned and not self._tile_is_listed(desc, self._tuned[key][0]):
                del self._tuned[key]                 # a remembered tile this build does not offer for this layer: time the layer again
            if key not in self._tuned:
                self._tuned[key] = self._time_tiles(plan, index, kind, desc, target, flops)
                fresh = True
            setattr(target, field, self._tuned[key][0])
            plan.tuning[name] = self._tuned[key]
            plan.tuning_parts.setdefault(name, []).append(self._tuned[key])
            if kind == OP_CONV and desc.tower_rows:
                # a layer of both forms: the dense tile was timed above (the lists' flag is 1 outside a run); the gathered tiles on a synthetic
                # list of every THIRD pixel -- between what real frames list and the crossover -- with the flag clear
                rows_key = (name + '@rows',) + key[1:]
                if rows_key in self._tuned and self._tuned[rows_key][0] not in self._tower_tiles(desc):
                    del self._tuned[rows_key]
                if rows_key not in self._tuned:
                    self._tuned[rows_key] = self._time_tower_tiles(plan, index, desc)
                    fresh = True
                desc.tower_tile = self._tuned[rows_key][0]
                plan.tuning[name + '@rows'] = self._tuned[rows_key]
        if plan.sparse is not None:
            for d in plan.sparse.deep:           # the same layer shape as the last layer: the tile its gathered launches were timed to
                d.deep_tile = plan.sparse.tower[0].tower_tile
            plan.sparse.reset(self.torch)
        self.torch.cuda.synchronize()
        if fresh:
            self._save_tune_cache()

    def _tile_choices(self, plan, index, kind, target):
        """ the tiles one op can take: the fused tail's row counts, the pre-activation conv's candidates, or the conv's candidates that its
        launcher accepts for this shape (a trial launch each: a candidate the launcher refuses is skipped, as the autotuner does) """
        if kind == OP_TAIL:
            return (64, 96, 128, 160) if self.dtype in C.X3_TYPES else (96, 128, 160)
        lib, tiles, count = hip.lib(), (ctypes.c_int * 32)(), ctypes.c_int(0)
        if kind == OP_MOBILENET_BLOCK:
            hip.check(lib.gpp_mobilenet_block_tile_candidates(ctypes.byref(target), tiles, 16, ctypes.byref(count)),
                      'gpp_mobilenet_block_tile_candidates')
            return list(tiles[:min(count.value, 16)])
        if kind == OP_CONV_PREACT:
            hip.check(lib.gpp_conv2d_preact_tile_candidates(ctypes.byref(target), tiles, 16, ctypes.byref(count)),
                      'gpp_conv2d_preact_tile_candidates')
            return list(tiles[:min(count.value, 16)])
        hip.check(lib.gpp_conv2d_tile_candidates(ctypes.byref(target), tiles, 32, ctypes.byref(count)), 'gpp_conv2d_tile_candidates')
        ok = []
        for tile in tiles[:count.value]:
            target.tile_hint = tile
            if lib.gpp_plan_run(ctypes.byref(plan.array, index * ctypes.sizeof(PlanOp)), 1, hip.stream_ptr(), None, 0) == 0:
                ok.append(tile)
        return ok

    def _time_tiles(self, plan, index, kind, desc, target, flops):
        """ (tile, us) of the fastest choice of one op: the fused tail's row counts timed here (GPP_TAIL64=0: not 64), the conv tiles by
        the library -- fewer launches per candidate for the float32 path, whose launches are 3 x as long (round 4: the x3 types on those
        counts rested a big layer's choice on four launches per candidate, and one tuning run in ~60 picked a tile that cost 5 %) """
        if kind == OP_TAIL:
            times = {}
            for rows in self._tile_choices(plan, index, kind, target):
                if rows == 64 and os.environ.get('GPP_TAIL64', '1') == '0':
                    continue
                desc.tile_rows = rows
                e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
                self.run_op(plan, index)
                e0.record()
                for _ in range(16):
                    self.run_op(plan, index)
                e1.record()
                e1.synchronize()
                times[rows] = e0.elapsed_time(e1) * 1000.0 / 16
            rows = min(times, key=times.get)
            return rows, round(times[rows], 2)
        slow = self.dtype == 'f32'
        iters = (2 if slow else 6) if flops > 5e10 else (4 if slow else 16)
        best = ctypes.c_float(0.0)
        if kind == OP_MOBILENET_BLOCK:
            hip.check(hip.lib().gpp_mobilenet_block_autotune(ctypes.byref(target), iters, hip.stream_ptr(), ctypes.byref(best)),
                      'gpp_mobilenet_block_autotune')
        elif kind == OP_CONV_PREACT:
            hip.check(hip.lib().gpp_conv2d_preact_autotune(ctypes.byref(target), desc.in_scale, desc.in_shift, iters, hip.stream_ptr(),
                                                           ctypes.byref(best)), 'gpp_conv2d_preact_autotune')
        else:
            hip.check(hip.lib().gpp_conv2d_autotune(ctypes.byref(target), iters, hip.stream_ptr(), ctypes.byref(best)), 'gpp_conv2d_autotune')
        return int(target.tile_hint), round(float(best.value), 2)

    @staticmethod
    def _tower_tiles(desc):
        """ the tiles the gathered launch of a layer of both forms may take: the library's candidates for the layer as a gathered one """
        rows = type(desc).from_buffer_copy(desc)
        rows.gather_rows, rows.gather_counts = desc.tower_rows, desc.tower_counts
        rows.tower_rows = rows.tower_counts = rows.tower_flag = None
        rows.tower_tile, rows.split_k = 0, 1
        tiles, count = (ctypes.c_int * 32)(), ctypes.c_int(0)
        hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(rows), tiles, 32, ctypes.byref(count)), 'gpp_conv2d_tile_candidates')
        return [t for t in tiles[:min(count.value, 32)] if t]

    def _time_tower_tiles(self, plan, index, desc, iters=8):
        """ (tile, us) of the fastest gathered tile of a layer of both forms, on every third pixel; the flag is 1 again afterwards """
        sp, torch = plan.sparse, self.torch
        sp.put_every_nth(torch, 3, tower=True)
        sp.tower_flag.fill_(0)
        times = {}
        for tile in self._tower_tiles(desc):
            desc.tower_tile = tile
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.run_op(plan, index)
            e0.record()
            for _ in range(iters):
                self.run_op(plan, index)
            e1.record()
            e1.synchronize()
            times[tile] = e0.elapsed_time(e1) * 1000.0 / iters
        sp.tower_flag.fill_(1)
        sp.tower_counts.zero_()
        tile = min(times, key=times.get)
        return tile, round(times[tile], 2)

    @staticmethod
    def _tile_is_listed(desc, tile):
        tiles, count = (ctypes.c_int * 64)(), ctypes.c_int(0)
        hip.check(hip.lib().gpp_conv2d_tile_candidates(ctypes.byref(desc), tiles, 64, ctypes.byref(count)), 'gpp_conv2d_tile_candidates')
        return int(tile) in list(tiles[:min(count.value, 64)])

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
        kind, _, desc, _, _ = plan.ops[index]
        if kind == OP_CONV and desc.lists_after:
            # the op has made the deep lists and set their flags; an op run on its own writes its whole map, so the
            # flags are 1 again behind it, ordered on the stream
            plan.sparse.reset_deep()

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
