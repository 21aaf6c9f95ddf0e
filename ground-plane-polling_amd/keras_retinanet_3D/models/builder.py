"""
The plan builder: one PlanBuilder lives for one RetinaNet3D._build call and records the plan of one (batch, H, W, N planes) -- it lays
out the activations, fills the descriptors of models/plan.py and emits the launches, stage by stage (build()).  What every stage needs --
the plan, its options, the batch and frame sizes, the map allocators, the pyramid layout, the decode descriptor -- is state of the builder;
which form a bottleneck or a head layer takes is decided by the pure rules of models/plan.py (block_form, head_forms) before anything is
emitted, and the methods here only follow them.  The model (models/retinanet.py) owns the weights and runs the plans.
"""

import ctypes

from ..backend import hip
from ..layers import conv as C
from ..layers import mobilenet as M
from ..layers.filter_detections import MAX_DETECTIONS, NMS_THRESHOLD, SCORE_THRESHOLD
from ..utils import anchors as anchor_utils
from ..utils import cuboid_nms as cuboid_nms_utils
from ..utils.gpp_utils import POLL_THRESHOLD, POSE_SCORE_THRESHOLD
from . import weights as W
from .plan import (BlockDesc, BlockProjDesc, CandidatePixelsDesc, CuboidNmsDesc, DensePoolDesc, DetectDesc, PollDesc, PoolDesc, PoseDesc,
                   PreactDesc, RaggedPoolDesc, RaggedStemDesc, ReluDesc, StemDesc, TailDesc,
                   OP_STEM, OP_MAXPOOL, OP_CONV, OP_RELU, OP_DETECT, OP_POLL, OP_TAIL, OP_BLOCK,
                   OP_DETECT_CANDIDATES, OP_DETECT_SELECT, OP_DETECT_EMIT, OP_DETECT_OSF, OP_STEM_POOL,
                   OP_MAXPOOL_PAD, OP_AVGPOOL, OP_CONV_PREACT, OP_MOBILENET_STEM, OP_MOBILENET_BLOCK, OP_POSE, OP_CUBOID_NMS,
                   OP_ABSMAX, OP_ABSMAX_CLEAR, OP_STEM_RAGGED, OP_STEM_POOL_RAGGED, OP_MAXPOOL_RAGGED, OP_DETECT_CANDIDATE_PIXELS,
                   block_form, head_forms, layer_split, part_of, TOWER_SLICES, TOWER0, TOWER0_SLICE, SparseHeads, Plan)


class PlanBuilder(object):
    """ builds the plan of `model` for B frames of H x Wd and n_planes road planes (ragged: the plan of a height class, RetinaNet3D._build) """

    def __init__(self, model, B, H, Wd, n_planes, planes_batched, ragged=False):
        torch, dev = model.torch, model.device
        self.model, self.torch, self.device = model, torch, dev
        self.B, self.H, self.Wd, self.n_planes, self.planes_batched = B, H, Wd, n_planes, planes_batched
        self.opts = opts = model._plan_options(B)
        self.plan = plan = Plan()
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
        # the pyramid layout (layout()) and the decode descriptor with what each decode launch reads and writes (detect())
        self.shapes = self.pix = self.total = None
        self.tower0 = None         # towers_0_split: (the regression slice's descriptor, the maps it reads, the maps it writes)
        self.detect_desc = self.detect_access = self.detect_all = None

    def build(self):
        m, plan = self.model, self.plan
        backbone = self.densenet_backbone if m.densenet else self.mobilenet_backbone if m.mobilenet else self.resnet_backbone
        C2, C3, C4, C5 = backbone()
        plan.features = {'stem': plan.stem_out, 'C2': C2, 'C3': C3, 'C4': C4, 'C5': C5}
        self.layout(C3, C4, C5)
        P = self.fpn(C3, C4, C5)
        plan.features.update({'P{}'.format(i + 3): P[i] for i in range(5)})
        outs = self.detect(self.anchor_table())
        self.heads(P, outs)
        self.poll()
        if m.pose:
            self.pose()
        if m.cuboid_nms is not None:
            self.cuboid_nms()
        if m.audit:
            self.audit()
        self.bind_workspaces()
        plan.finalize()
        plan.tagged = [name for _, tag, _, name, _ in plan.ops if tag]
        return plan

    # ------------------------------------------------------------------ maps
    def fmap(self, h, w, c, split=False):
        """ a dense map of the whole batch in the storage type; bmap / smap: pre-split where the plan stores the backbone's / the FPN's maps so """
        m = self.model
        f = C.FMap.empty(self.B, h, w, c, m.tdtype, self.device, half=m.dtype if m.dtype in C.X3_TYPES else 'bf16x3')
        self.plan.keep.append(f.buf)
        return f.mark_split() if split else f

    def bmap(self, h, w, c):
        return self.fmap(h, w, c, self.opts.x3_level >= 2)

    def smap(self, h, w, c):
        return self.fmap(h, w, c, self.opts.x3_level >= 1)

    def anchor_table(self):
        """ the anchors of this frame size on the device, kept by the model; a DenseNet's follow its own level shapes """
        m, hw = self.model, (self.H, self.Wd)
        key = (hw, tuple(self.shapes)) if m.densenet else hw
        if key not in m._anchors:
            a = anchor_utils.anchors_for_shapes(self.shapes) if m.densenet else anchor_utils.anchors_for_image(hw)
            m._anchors[key] = self.torch.as_tensor(a).to(self.device).contiguous()
        return m._anchors[key]

    # ------------------------------------------------------------------ launches
    def desc(self, name, inputs, outputs, K, stride=1, pad=None, relu=False, residuals=None, out_f32=False, lane=0):
        m, plan = self.model, self.plan
        wt, bias, shape = m.conv_w[name]
        kh, kw, cin, cout = shape
        if pad is None:
            pad = (0, 0)
        # plan='latency': an explicit split-K factor per layer (a function of the layer alone); 0 = the library's own rule
        split = layer_split(m.plan_mode, shape, sum(f.H * f.W for f in outputs)) if m.plan_mode == 'latency' else 0
        d = C.conv_desc(inputs, outputs, wt, bias, kh, kw, cin, cout, stride=stride, pad=pad, relu=relu,
                        residuals=residuals, dtype=m.dtype, out_f32=out_f32, out_scale=m.conv_scale.get(name), split_k=split)
        if m.dtype == 'f16x3':         # this plan's own range-event slot (Plan.range_slot): what its launches count no other plan sees
            d.range_counter = plan.range_slot.data_ptr()
        # split-K partial tiles: the workspace of this op's stream lane is allocated once every op is known (bind_workspaces)
        plan.conv_descs.append((d, lane))
        plan.ws_need[lane] = max(plan.ws_need.get(lane, 0), C.workspace_bytes(d))
        return d

    def conv(self, name, inputs, outputs, K, stride=1, pad=None, relu=False, residuals=None, out_f32=False, tag=0, lane=0,
             join=False, sync=False):
        d = self.desc(name, inputs, outputs, K, stride, pad, relu, residuals, out_f32, lane)
        self.plan.emit(OP_CONV, d, name, list(inputs) + list(residuals or []), outputs, tag=tag, flops=C.conv_flops(d), lane=lane, join=join,
                       sync=sync, io=(inputs, outputs, residuals))

    def tail(self, nm, a, y, shortcut, join=False, lane=0):
        """ branch2b (3x3) + branch2c (1x1, + shortcut, ReLU) of one bottleneck as ONE launch
        (gpp_bottleneck_tail): the intermediate map never reaches HBM.  Bit-identical to the two layers. """
        d1 = self.desc('res{}_branch2b'.format(nm), [a], [a], 3, pad=(1, 1), relu=True)       # its `out` is never written
        d2 = self.desc('res{}_branch2c'.format(nm), [a], [y], 1, relu=True, residuals=[shortcut])
        self.plan.emit(OP_TAIL, TailDesc(ctypes.addressof(d1), ctypes.addressof(d2), 0, 0), 'res{}_branch2b+2c'.format(nm), [a, shortcut], [y],
                       flops=C.conv_flops(d1) + C.conv_flops(d2), join=join, lane=lane, io=([a], [y], [shortcut]), inner=(d1, d2))

    def block(self, nm, x, a, bmap, y, shortcut, stride=1, join=False, lane=0):
        """ a whole bottleneck -- branch2a, branch2b, branch2c (+ shortcut, ReLU) -- as ONE launch (gpp_bottleneck_block): neither intermediate map
        reaches HBM (`a` / `bmap` only lend the descriptors their shapes).  Bit-identical to the three layers. """
        d1 = self.desc('res{}_branch2a'.format(nm), [x], [a], 1, stride=stride, relu=True)
        d2 = self.desc('res{}_branch2b'.format(nm), [a], [bmap], 3, pad=(1, 1), relu=True)
        d3 = self.desc('res{}_branch2c'.format(nm), [bmap], [y], 1, relu=True, residuals=[shortcut])
        t = BlockDesc(ctypes.addressof(d1), ctypes.addressof(d2), ctypes.addressof(d3), 0, 0)
        self.plan.emit(OP_BLOCK, t, 'res{}_branch2a+2b+2c'.format(nm), [x, shortcut], [y], flops=C.conv_flops(d1) + C.conv_flops(d2) + C.conv_flops(d3),
                       join=join, lane=lane, io=([x], [y], [shortcut]), inner=(d1, d2, d3))

    def block_proj(self, nm, x, a, bmap, sc, y, join=False, lane=0):
        """ a whole projection bottleneck -- branch2a, branch1, branch2b, branch2c (+ shortcut, ReLU) -- as ONE launch (gpp_bottleneck_block_proj): the
        shortcut is computed from the input rows branch2a stages and never becomes a map (`a` / `bmap` / `sc` only lend the descriptors their
        shapes).  Bit-identical to the four layers. """
        d1 = self.desc('res{}_branch2a'.format(nm), [x], [a], 1, relu=True)
        d2 = self.desc('res{}_branch2b'.format(nm), [a], [bmap], 3, pad=(1, 1), relu=True)
        d3 = self.desc('res{}_branch2c'.format(nm), [bmap], [y], 1, relu=True)
        dp = self.desc('res{}_branch1'.format(nm), [x], [sc], 1)
        t = BlockProjDesc(ctypes.addressof(d1), ctypes.addressof(d2), ctypes.addressof(d3), 0, 1, ctypes.addressof(dp))
        self.plan.emit(OP_BLOCK, t, 'res{}_branch2a+2b+2c'.format(nm), [x], [y],
                       flops=C.conv_flops(d1) + C.conv_flops(d2) + C.conv_flops(d3) + C.conv_flops(dp), join=join, lane=lane, io=([x], [y], None),
                       inner=(d1, d2, d3, dp))

    def preact(self, name, inputs, outputs, relu=False):
        """ a 1x1 conv behind its input's BatchNormalization + ReLU (gpp_conv2d_preact): DenseNet's _1_conv and transition convs """
        d = self.desc(name, inputs, outputs, 1, relu=relu)
        s, t = self.model.preact[name]
        self.plan.emit(OP_CONV_PREACT, PreactDesc(ctypes.addressof(d), s.data_ptr(), t.data_ptr()), name, inputs, outputs, flops=C.conv_flops(d),
                       io=(inputs, outputs, None), inner=(d,))

    # ------------------------------------------------------------------ backbones
    def stem(self, x):
        """ conv1 + bn + relu (7x7 / 2) and pool1 (3x3 / 2) into x.  opts.fuse_stem_pool: one launch, the (B, H1, W1, 64) conv map is never
        stored (bit-identical to the two launches: tests/test_stem_gpu.py; 16-bit types since round 2, the x3 types since round 6 --
        gpp_stem_pool_fused_x3: the float32 conv map was 274 MB written + read back at B = 8).  Else the conv map is stored and pooled by a
        second launch: ResNet's max pool, or DenseNet's zero-padded one into the channel prefix of its first concatenation buffer. """
        m, plan, opts, B, H, Wd = self.model, self.plan, self.opts, self.B, self.H, self.Wd
        H1, W1 = (H + 6 - 7) // 2 + 1, (Wd + 6 - 7) // 2 + 1
        conv = x if opts.fuse_stem_pool else self.fmap(H1, W1, 64)
        d = StemDesc(plan.images.data_ptr(), m.stem_w.data_ptr(), m.stem_b.data_ptr(), conv.buf.data_ptr(),
                     hip.GPP_F16X3 if m.stem_x3 else C.gpp_storage_dtype(m.dtype), B, H, Wd,
                     plan.range_slot.data_ptr() if m.dtype == 'f16x3' else None)
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
            pd = RaggedPoolDesc(PoolDesc(conv.buf.data_ptr(), x.buf.data_ptr(), C.gpp_storage_dtype(m.dtype), B, H1, W1, 64, 0),
                                plan.heights.data_ptr(), x.H, 0)
            plan.emit(OP_MAXPOOL_RAGGED, pd, 'pool1', [conv, plan.heights], [C.FMap(x.buf, B, x.H, x.W, 64, pitch=x.pitch)])
            return
        if opts.fuse_stem_pool:
            plan.emit(OP_STEM_POOL, d, 'conv1+pool1', [plan.images], [x], flops=flops)
            return
        plan.emit(OP_STEM, d, 'conv1', [plan.images], [conv], flops=flops)
        pooled = C.FMap(x.buf, B, x.H, x.W, 64, pitch=x.pitch)
        if m.densenet:
            pd = DensePoolDesc(conv.buf.data_ptr(), x.buf.data_ptr(), B, H1, W1, 64, 1, x.pitch)
            plan.emit(OP_MAXPOOL_PAD, pd, 'pool1', [conv], [pooled])
        else:
            pd = PoolDesc(conv.buf.data_ptr(), x.buf.data_ptr(), C.gpp_storage_dtype(m.dtype), B, H1, W1, 64, 0)
            plan.emit(OP_MAXPOOL, pd, 'pool1', [conv], [pooled])

    def resnet_backbone(self):
        """ conv1 .. res5 of keras_resnet (bottleneck_2d: stride on the first 1x1) -> [C2, C3, C4, C5].  A stage runs as two half
        batches (opts.half_stages), the second half on side lane 1 beside the first, or chunk of images by chunk of images
        (opts.stage_chunks), one chunk after the other; the halves stay apart until the next whole-batch launch joins them. """
        plan, opts, B, bmap, name = self.plan, self.opts, self.B, self.bmap, self.model.backbone_name
        H1, W1 = (self.H + 6 - 7) // 2 + 1, (self.Wd + 6 - 7) // 2 + 1
        x = self.fmap((H1 + 1) // 2, (W1 + 1) // 2, 64)
        self.stem(x)
        feats = []
        for stage, n_blocks in enumerate(W.BLOCKS[name]):
            f, xin, blocks = 64 * 2 ** stage, x, []
            for block in range(n_blocks):
                stride = 2 if (block == 0 and stage > 0) else 1
                ho, wo = (x.H - 1) // stride + 1, (x.W - 1) // stride + 1
                # (fused tails have no branch2b map: a fused block's descriptors borrow branch2a's -- neither is written)
                a, b = bmap(ho, wo, f), None if f in opts.fuse_tail else bmap(ho, wo, f)
                sc = bmap(ho, wo, 4 * f) if block == 0 else None
                x = bmap(ho, wo, 4 * f)
                blocks.append((W.block_name(name, stage, block), stride, a, b, sc, x))
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
                self.bottleneck(nm, form, stride, xs, part_of(a, c0, nb), b and part_of(b, c0, nb),
                                part_of(sc, c0, nb) if sc else xs, xs_of[c0], lane, join)
            feats.append(x)
        return feats

    def bottleneck(self, nm, form, stride, x, a, b, sc, y, lane, join):
        """ one bottleneck (of one batch part) in the form block_form chose.  join: its first launch closes the side lanes of the stage
        before; a projection shortcut on side lane 1 is joined by the launch that adds it. """
        launch, shortcut = form
        branch1 = 'res{}_branch1'.format(nm)
        if shortcut == 'inproj':
            self.block_proj(nm, x, a, b or a, sc, y, join=join, lane=lane)
            return
        if shortcut == 'side':
            self.conv(branch1, [x], [sc], 1, stride=stride, lane=1)
        if launch == 'block':
            if shortcut == 'inline':         # a projection block: the shortcut map first, in line, then the whole block
                self.conv(branch1, [x], [sc], 1, stride=stride, lane=lane, join=join)
                join = False
            self.block(nm, x, a, b or a, y, sc, stride=stride, join=join or shortcut == 'side', lane=lane)
            return
        self.conv('res{}_branch2a'.format(nm), [x], [a], 1, stride=stride, relu=True, lane=lane, join=join)
        if shortcut == 'inline':
            self.conv(branch1, [x], [sc], 1, stride=stride, lane=lane)
        if launch == 'tail':
            self.tail(nm, a, y, sc, join=shortcut == 'side', lane=lane)
        else:
            self.conv('res{}_branch2b'.format(nm), [a], [b], 3, pad=(1, 1), relu=True, lane=lane)
            self.conv('res{}_branch2c'.format(nm), [b], [y], 1, relu=True, residuals=[sc], join=shortcut == 'side', lane=lane)

    def densenet_backbone(self):
        """ conv1 .. conv5_block{N}_concat of keras' DenseNet (reference models/densenet.py:62-94) -> the four block concatenations.
        One float32 buffer per dense block at its final width: the block input (pool1 / the transition's average pool) is written into
        channels [0, C0), layer I's 32 channels into [C0 + 32 (I - 1), C0 + 32 I), and layer I's _1_conv reads the prefix [0, C0 + 32 (I - 1))
        through in_pitch.  The 128-channel map between _1_conv and _2_conv is pre-split for the x3 types.  The whole batch on lane 0. """
        B, name = self.B, self.model.backbone_name
        widths = W.densenet_widths(name)
        H1, W1 = (self.H + 6 - 7) // 2 + 1, (self.Wd + 6 - 7) // 2 + 1
        h, w = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        cats = []
        for stage in range(4):
            cats.append(self.fmap(h, w, widths[stage]))
            h, w = h // 2, w // 2
        self.stem(cats[0])
        c0 = 64
        for stage, n in enumerate(W.DENSENET_BLOCKS[name]):
            cat = cats[stage]
            for i in range(1, n + 1):
                nm = 'conv{}_block{}'.format(stage + 2, i)
                cin = c0 + W.DENSENET_GROWTH * (i - 1)
                mid = self.bmap(cat.H, cat.W, W.DENSENET_BOTTLENECK)
                self.preact(nm + '_1_conv', [C.FMap(cat.buf, B, cat.H, cat.W, cin, pitch=cat.pitch)], [mid], relu=True)
                self.conv(nm + '_2_conv', [mid], [C.FMap(cat.buf, B, cat.H, cat.W, W.DENSENET_GROWTH, off=cin, pitch=cat.pitch)], 3,
                          pad=(1, 1))
            if stage == 3:
                break
            nm = 'pool{}'.format(stage + 2)
            t = self.fmap(cat.H, cat.W, widths[stage] // 2)
            self.preact(nm + '_conv', [cat], [t])
            nxt = cats[stage + 1]
            pd = DensePoolDesc(t.buf.data_ptr(), nxt.buf.data_ptr(), B, t.H, t.W, t.C, 0, nxt.pitch)
            self.plan.emit(OP_AVGPOOL, pd, nm + '_pool', [t], [C.FMap(nxt.buf, B, nxt.H, nxt.W, t.C, pitch=nxt.pitch)])
            c0 = t.C
        return cats

    def mobilenet_backbone(self):
        """ conv1 .. conv_pw_13_relu of keras' MobileNet (reference models/mobilenet.py:94-111) -> conv_pw_3 / 5 / 11 / 13 behind their
        ReLU6 (C2 .. C5).  conv1 is one launch (gpp_mobilenet_stem), every depthwise-separable block ONE launch (gpp_mobilenet_block: the
        depthwise map never reaches HBM).  Every map is float32, never pre-split; the whole batch on lane 0. """
        m, plan, B, H, Wd = self.model, self.plan, self.B, self.H, self.Wd
        c0 = W.mobilenet_filters(m.backbone_name)[0]
        x = self.fmap(M.out_size(H, 2), M.out_size(Wd, 2), c0)
        sd = hip.MobileNetStemDesc(plan.images.data_ptr(), m.stem_w.data_ptr(), m.stem_b.data_ptr(), x.buf.data_ptr(), B, H, Wd, c0, x.pitch, 0)
        plan.stem_out, plan.pool_out = x, None
        plan.emit(OP_MOBILENET_STEM, sd, 'conv1', [plan.images], [x], flops=2.0 * B * x.H * x.W * 27 * c0)
        feats = []
        for i, cin, cout, stride in W.mobilenet_blocks(m.backbone_name):
            y = self.fmap(M.out_size(x.H, stride), M.out_size(x.W, stride), cout)
            dw_w, dw_b, pw_w, pw_b, scale = m.mbn_w[i]
            d = M.block_desc(x, y, dw_w, dw_b, pw_w, pw_b, scale, stride, m.dtype)
            plan.emit(OP_MOBILENET_BLOCK, d, 'conv_pw_{}'.format(i), [x], [y], flops=M.block_flops(d), io=([x], [y], None))
            x = y
            if i in W.MOBILENET_TAPS:
                feats.append(x)
        return feats

    # ------------------------------------------------------------------ pyramid
    def layout(self, C3, C4, C5):
        """ the layout of every FPN / head tensor: the five levels back to back per image, (B, sum(H_l*W_l), C), so that one grouped
        launch covers all levels; a DenseNet's pyramid has the sizes of its own C3 .. C5 (floor pools).  Sets shapes (of the levels), pix
        (pixels per level) and total (pixels per image), which pyramid() lays tensors out by. """
        got = [(C3.H, C3.W), (C4.H, C4.W), (C5.H, C5.W)]
        shapes = anchor_utils.pyramid_shapes_of_features(got) if self.model.densenet else anchor_utils.pyramid_shapes((self.H, self.Wd))
        if got != [tuple(s) for s in shapes[:3]]:
            raise RuntimeError('backbone / pyramid shape mismatch: {} vs {}'.format(got, shapes))
        self.shapes, self.pix = shapes, [h * w for h, w in shapes]
        self.total = sum(self.pix)
        self.plan.n_anchors = self.total * anchor_utils.NUM_BASE_ANCHORS

    def pyramid(self, c, dtype=None):
        """ a pyramid tensor of c channels (dtype: float32 head outputs; default: the storage type, pre-split where the plan stores the
        FPN's maps so) -> (buffer, its five level FMaps) """
        m, B, pix, total = self.model, self.B, self.pix, self.total
        buf = self.torch.empty((B, total, c), dtype=dtype or m.tdtype, device=self.device)
        self.plan.keep.append(buf)
        sp = self.opts.x3_level >= 1 and dtype is None
        return buf, [C.FMap(buf, B, h, w, c, off=sum(pix[:i]) * c, bstride=total * c, split=sp, half=m.dtype if sp else 'bf16x3')
                     for i, (h, w) in enumerate(self.shapes)]

    def fpn(self, C3, C4, C5):
        """ P3 .. P7 into one pyramid tensor (512 channels); returns its five level maps.  P5 and the P6 -> ReLU -> P7 chain are small
        launches (a few dozen tiles) independent of the C4 / C3 chain: with opts.fpn_lanes they run on the side streams underneath the
        C4_reduced / P4 launches (182 workgroups each: 74 CUs idle), joined by the fused first tower layer (measured +0.8 % on the f16x3
        step).  P4 (182 workgroups of 192 x 256: 71 % of the CUs) only feeds the towers: with opts.p4_lane it runs behind P5 on its side
        stream (re-forked: it needs T4), beside C3_reduced / P3. """
        plan, opts, smap, esz = self.plan, self.opts, self.smap, self.model.esz
        _, P = self.pyramid(512)
        l_p5, l_p6 = (1, 2) if opts.fpn_lanes else (0, 0)
        T5 = smap(C5.H, C5.W, 512)
        self.conv('C5_reduced', [C5], [T5], 1, join=bool(plan.open_lanes))
        self.conv('P5', [T5], [P[2]], 3, pad=(1, 1), lane=l_p5)
        self.conv('P6', [C5], [P[3]], 3, stride=2, pad=(C.same_pad(C5.H, 3, 2)[1], C.same_pad(C5.W, 3, 2)[1]), lane=l_p6)
        R6 = smap(P[3].H, P[3].W, 512)
        relu_d = ReluDesc(P[3].buf.data_ptr() + P[3].off * esz, R6.buf.data_ptr(), P[3].bstride, R6.bstride, P[3].H * P[3].W * 512,
                          C.gpp_dtype(self.model.dtype) if opts.x3_level >= 1 else C.gpp_storage_dtype(self.model.dtype), P[3].B)
        plan.emit(OP_RELU, relu_d, 'C6_relu', [P[3]], [R6], lane=l_p6)
        plan.relu_io = (P[3], R6)
        self.conv('P7', [R6], [P[4]], 3, stride=2, pad=(C.same_pad(P[3].H, 3, 2)[1], C.same_pad(P[3].W, 3, 2)[1]), lane=l_p6)
        T4 = smap(C4.H, C4.W, 512)
        self.conv('C4_reduced', [C4], [T4], 1, residuals=[T5])          # + UpsampleLike(P5, C4), fused
        self.conv('P4', [T4], [P[1]], 3, pad=(1, 1), lane=opts.p4_lane, sync=bool(opts.p4_lane))
        T3 = smap(C3.H, C3.W, 512)
        self.conv('C3_reduced', [C3], [T3], 1, residuals=[T4])          # + UpsampleLike(P4, C3), fused
        self.conv('P3', [T3], [P[0]], 3, pad=(1, 1))
        return P

    # ------------------------------------------------------------------ decode
    def detect(self, anchors):
        """ decode + NMS (RegressBoxes, RegressDims, FilterDetections): the three head outputs (float32 pyramids), the detection outputs,
        the workspace and the one descriptor the decode launches share (decode()), allocated before the towers are emitted.
        Returns the (classification, regression, dimension) output maps. """
        m, plan, B, torch, dev, D = self.model, self.plan, self.B, self.torch, self.device, MAX_DETECTIONS
        f32, i32 = torch.float32, torch.int32
        plan.cls_logits, cls_o = self.pyramid(96, f32)
        plan.regression, reg_o = self.pyramid(144, f32)
        plan.regression_dim, dim_o = self.pyramid(36, f32)
        plan.boxes = torch.empty((B, D, 12), dtype=f32, device=dev)
        plan.dimensions = torch.empty((B, D, 3), dtype=f32, device=dev)
        plan.scores = torch.empty((B, D), dtype=f32, device=dev)
        plan.labels = torch.empty((B, D), dtype=i32, device=dev)
        plan.orientations = torch.empty((B, D), dtype=i32, device=dev)
        plan.anchor_index = torch.empty((B, D), dtype=i32, device=dev)
        plan.counts = torch.zeros((B,), dtype=i32, device=dev)
        need = hip.c_size_t(0)
        if m.osf and B > 16:
            raise ValueError('orientation_specific_filter=True handles at most 16 images per batch')
        size_fn = hip.lib().gpp_detect_osf_workspace_bytes if m.osf else hip.lib().gpp_detect_workspace_bytes
        hip.check(size_fn(B, plan.n_anchors, need), 'gpp_detect_workspace_bytes')
        plan.detect_ws = ws = torch.empty((int(need.value),), dtype=torch.uint8, device=dev)
        plan.anchors = anchors
        self.detect_desc = DetectDesc(plan.cls_logits.data_ptr(), plan.regression.data_ptr(), plan.regression_dim.data_ptr(),
                                      anchors.data_ptr(), plan.boxes.data_ptr(), plan.dimensions.data_ptr(), plan.scores.data_ptr(),
                                      plan.labels.data_ptr(), plan.orientations.data_ptr(), plan.anchor_index.data_ptr(),
                                      plan.counts.data_ptr(), ws.data_ptr(), ws.numel(), plan.n_anchors,
                                      B, anchor_utils.NUM_BASE_ANCHORS, 1, D, SCORE_THRESHOLD, NMS_THRESHOLD if m.nms else 2.0)
        heads = [plan.cls_logits, plan.regression, plan.regression_dim]
        dets = [plan.boxes, plan.dimensions, plan.scores, plan.labels, plan.orientations, plan.anchor_index]
        self.detect_access = {OP_DETECT_CANDIDATES: ([plan.cls_logits], [ws, plan.counts]), OP_DETECT_SELECT: ([ws, plan.regression], [ws]),
                              OP_DETECT_EMIT: (heads + [ws], dets)}
        self.detect_all = (heads, dets + [ws, plan.counts])          # (OP_DETECT / OP_DETECT_OSF: the whole decode)
        return cls_o, reg_o, dim_o

    def decode(self, kind, name='filtered_detections', **flags):
        """ records one decode launch on the descriptor of detect() """
        plan, dd, ws = self.plan, self.detect_desc, self.plan.detect_ws
        reads, writes = self.detect_access.get(kind, self.detect_all)
        if kind == OP_DETECT_CANDIDATE_PIXELS:      # the candidate pass + the pixel lists of the gathered head output layers, one op
            sp = plan.sparse
            lists = hip.PixelListDesc(ws.data_ptr(), sp.bitmap.data_ptr(), sp.rows.data_ptr(), sp.counts.data_ptr(), sp.flag.data_ptr(),
                                      plan.n_anchors, self.B, anchor_utils.NUM_BASE_ANCHORS, 4 if self.model.osf else 1, len(sp.level_pixels),
                                      sp.max_rows, 0, (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*sp.level_pixels), 0)
            if sp.tower_rows is not None:       # ... and their 3 x 3 dilation: what the regression tower's last layer has to write
                lists.dilated_bitmap, lists.dilated_rows = sp.tower_bitmap.data_ptr(), sp.tower_rows.data_ptr()
                lists.dilated_counts, lists.dilated_flag = sp.tower_counts.data_ptr(), sp.tower_flag.data_ptr()
                lists.level_width = (ctypes.c_int32 * hip.GPP_MAX_GROUPS)(*sp.level_widths)
                lists.dilated_max_rows = sp.tower_max_rows
            reads, writes = self.detect_access[OP_DETECT_CANDIDATES]
            plan.emit(kind, CandidatePixelsDesc(ctypes.addressof(dd), lists), name, reads, writes + sp.tensors(), inner=(dd,), **flags)
            return
        plan.emit(kind, dd, name, reads, writes, **flags)

    # ------------------------------------------------------------------ heads
    def heads(self, P, outs):
        """ the three towers (every layer one grouped launch over the five levels; layer 0 of the three shares its input: one fused
        launch, C_out = 896, whose channel slices layers 1..3 read) and the decode launches where their inputs are complete.
        opts.decode_overlap: classification, regression, dimension tower; the detection selection (one workgroup per image, 8 of the
        256 CUs) only needs the logits and the corner regressions, so it runs on a side stream underneath the dimension tower, and the
        decode of the <= 100 survivors joins when every head is done.  opts.head_lanes: the two small towers on side streams, filling
        the ramp-up / tail phases of the big regression-tower kernels.  opts.cls_lane: the classification tower (+ the candidate pass)
        on side lane 2 BESIDE the regression tower, whose last layer joins it.  Which layers take a sparse form is head_forms' answer (models/plan.py); the methods below follow it. """
        m, plan, opts = self.model, self.plan, self.opts
        cls_o, reg_o, dim_o = outs
        _, wide = self.pyramid(896)
        names = ('pyramid_classification', 'pyramid_regression_ops', 'pyramid_regression_dim', 'pyramid_regression_1', 'pyramid_regression_2',
                 'pyramid_regression_3', TOWER0)
        forms = head_forms(opts, m.dtype, m.plan_mode, m.osf, m.audit, {n: m.conv_w[n][2] for n in names},
                           hasattr(hip.lib(), 'gpp_detect_deep_lists'), self.shapes, self.B, hasattr(hip.lib(), 'gpp_conv2d_deferred_register'))
        if forms.sparse:
            plan.sparse = SparseHeads(self.torch, self.device, self.B, [f.H * f.W for f in P], opts.sparse_heads, [f.W for f in P],
                                      opts.sparse_tower if forms.tower_both else 0.0)
            plan.keep += plan.sparse.tensors()
            if forms.deep_layers:
                plan.sparse.add_deep(self.torch, forms.deep_layers, opts.sparse_deep)
                plan.keep += plan.sparse.deep_tensors()
            if forms.tower0:
                plan.sparse.add_tower0(self.torch)
                plan.keep += plan.sparse.tower0_tensors()
        # (measured and rejected: the half-empty fourth 256-column tile of this 896-wide layer as its own 128-column launch
        # on a side stream -- the two launches do not pack into each other's partial rounds, no gain)
        if forms.tower0:
            self.towers_0_split(P, wide)
        else:
            self.conv(TOWER0, P, wide, 3, pad=(1, 1), relu=True, join=True)
        l_dim, l_cls = (1, 2) if opts.head_lanes else (0, 0)
        towers = {'cls': ('pyramid_classification', 256, 512, 'pyramid_classification', cls_o, 0, l_cls or opts.cls_lane),
                  'reg': ('pyramid_regression', 512, 0, 'pyramid_regression_ops', reg_o, 1, 0, bool(opts.cls_lane)),
                  'dim': ('pyramid_regression_dim', 128, 768, 'pyramid_regression_dim', dim_o, 0, l_dim)}
        if opts.decode_overlap:
            self.tower(forms, wide, *towers['cls'])
            self.decode(OP_DETECT_CANDIDATE_PIXELS if plan.sparse else OP_DETECT_CANDIDATES, 'filtered_detections/candidates',
                        lane=opts.cls_lane or 1)     # on the tower's lane when it has one
            self.tower(forms, wide, *towers['reg'])
            self.decode(OP_DETECT_SELECT, 'filtered_detections/select', lane=1, sync=True)
            self.tower(forms, wide, *towers['dim'])
            self.decode(OP_DETECT_EMIT, join=True)
        else:
            for t in ('dim', 'cls', 'reg'):
                self.tower(forms, wide, *towers[t])
            self.decode(OP_DETECT_OSF if m.osf else OP_DETECT, join=True)

    def towers_0_split(self, P, wide):
        """ the fused first layer of the three towers in a plan whose regression tower is gathered down to layer 1 (head_forms: tower0).
        Columns [0, TOWER0_SLICE) of its map are layer 0 of the regression tower, and their only reader, the gathered layer 1, takes them on
        the 3 x 3 halo of its own rows: the 9 x 9 dilation of the candidates' pixels.  Those rows are known once the logits are, so the
        slice leaves this launch: the op computes the other columns (the classification and dimension slices, contiguous; the packed
        weights, the bias and the scale are addressed by a row offset: 512 is a multiple of the 32-row interleave), and the slice becomes a
        layer of both forms on the radius-4 lists that the library enqueues behind pyramid_classification's lists (out_layer:
        gpp_conv_desc.conv_after).  Still ONE op under this name with the algorithmic FLOPs of all columns and the whole map as its io:
        RetinaNet3D.run_op writes every column, as an op run on its own does. """
        m, plan, sp = self.model, self.plan, self.plan.sparse
        wt, bias, (kh, kw, cin, cout) = m.conv_w[TOWER0]
        scale = m.conv_scale.get(TOWER0)
        n = TOWER0_SLICE

        def cols(c0, c):
            return [C.FMap(f.buf, f.B, f.H, f.W, c, off=f.off + c0, bstride=f.bstride, pitch=f.pitch, split=f.split, half=f.half) for f in wide]

        def desc(c0, c):
            parts = [wt[c0:], bias[c0:]] + ([scale[c0:]] if scale is not None else [])
            plan.keep += parts
            d = C.conv_desc(P, cols(c0, c), parts[0], parts[1], kh, kw, cin, c, pad=(1, 1), relu=True, dtype=m.dtype,
                            out_scale=parts[2] if scale is not None else None)
            if m.dtype == 'f16x3':
                d.range_counter = plan.range_slot.data_ptr()
            return d
        rest = desc(n, cout - n)
        plan.conv_descs.append((rest, 0))
        plan.ws_need[0] = max(plan.ws_need.get(0, 0), C.workspace_bytes(rest))
        # (the slice never splits -- head_forms asked the rule -- and carries no workspace: the library's copy is made before any is bound)
        first = desc(0, n)
        first.weight_rows = n
        first.deep_rows, first.deep_counts, first.deep_flag = sp.tower0_rows.data_ptr(), sp.tower0_counts.data_ptr(), sp.tower0_flag.data_ptr()
        plan.keep.append(first)
        plan.emit(OP_CONV, rest, TOWER0, list(P), cols(n, cout - n), flops=C.conv_flops(rest) + C.conv_flops(first), join=True, io=(P, wide, None))
        self.tower0 = (first, list(P), cols(0, n))

    def tower(self, forms, wide, prefix, width, c0, out_name, out, tag=0, lane=0, join=False):
        """ layers 1 .. 3 of one tower on its `width` channels from c0 of the fused first layer's map, then its output layer.  The regression
        tower's layers take the forms head_forms named: the last `deep_layers` in front of layer 3 both forms, layer 3 too with tower_both """
        src = [C.FMap(f.buf, f.B, f.H, f.W, width, off=f.off + c0, bstride=f.bstride, pitch=f.pitch, split=f.split, half=f.half) for f in wide]
        regression = out_name == 'pyramid_regression_ops'
        for i in range(1, 4):
            name = '{}_{}'.format(prefix, i)
            _, dst = self.pyramid(width)
            if regression and i == 3 and forms.tower_both:
                self.tower_last(name, src, dst, tag, lane)
            elif regression and 3 - forms.deep_layers <= i < 3:
                self.tower_deep(name, src, dst, tag, lane, 2 - i)
            else:
                self.conv(name, src, dst, 3, pad=(1, 1), relu=True, tag=tag, lane=lane)
            src = dst
        self.out_layer('dense' if lane else forms.outputs[out_name], out_name, src, out, lane, join)

    def tower_last(self, name, src, dst, tag, lane):
        """ the regression tower's last layer where its only reader is the gathered output layer (head_forms: tower_both): that launch
        reads the map at the listed pixels and their eight neighbours, so this layer has to write the 3 x 3 dilation of the lists and
        nothing else.  ONE op (its flops the algorithmic count, its tag the tower's): gpp_conv2d_igemm enqueues the dense launch and the
        gathered one on the dilated lists (gpp_conv_desc.tower_rows), and the lists' flag lets exactly one of them work -- the dense one
        whenever the output layer runs dense, which reads every row.  The op joins the candidates' lane: it is the first reader of the
        lists.  The rows nobody reads keep whatever the buffer held; Plan.complete_heads runs the layer dense before anyone reads more. """
        sp = self.plan.sparse
        d = self.desc(name, src, dst, 3, pad=(1, 1), relu=True, lane=lane)
        d.tower_rows, d.tower_counts, d.tower_flag = sp.tower_rows.data_ptr(), sp.tower_counts.data_ptr(), sp.tower_flag.data_ptr()
        self.plan.emit(OP_CONV, d, name, list(src) + [sp.tower_rows, sp.tower_counts, sp.tower_flag], dst, tag=tag, flops=C.conv_flops(d), lane=lane,
                       join=not sp.lists_joined, io=(src, dst, None))
        sp.lists_joined = True
        sp.tower.append(d)

    def tower_deep(self, name, src, dst, tag, lane, which):
        """ layers 2 (which = 0) and 1 (which = 1) of the regression tower in a plan of the deep form (head_forms: deep_layers): the
        only reader of layer 2 is the gathered layer 3, which reads it on the 5 x 5 neighbourhoods of the candidates' pixels, and layer 1
        is read by the gathered layer 2 on the 7 x 7 ones.  ONE op each, as tower_last; the lists (gpp_conv_desc.deep_rows) come from
        gpp_detect_deep_lists behind pyramid_classification on this same stream, so there is no lane to join """
        sp = self.plan.sparse
        d = self.desc(name, src, dst, 3, pad=(1, 1), relu=True, lane=lane)
        lists = [sp.deep_rows[which], sp.deep_counts[which], sp.deep_flags[which]]
        d.deep_rows, d.deep_counts, d.deep_flag = [t.data_ptr() for t in lists]
        self.plan.emit(OP_CONV, d, name, list(src) + lists, dst, tag=tag, flops=C.conv_flops(d), lane=lane, io=(src, dst, None))
        sp.deep.append(d)

    def out_layer(self, form, name, src, out, lane, join):
        """ the output layer of a tower in the form head_forms named -- 'dense' on a side lane, whatever it named (tower()).
        'pair': the decode reads these maps at candidate anchors only (nms_kernel, emit_kernel), and the candidate lists exist before the
        regression tower starts -- so the layer runs in gathered-row form on the pixels gpp_detect_pixel_lists listed
        (gpp_conv_desc.gather_rows: byte-identical rows, nothing else written).  The dense launch stays in the plan in front of it, guarded
        by the lists' flag: when more than max_rows rows are listed it runs and the gathered one returns at once, otherwise all its
        workgroups return on the flag -- no host round trip either way.  The first of the pair joins the candidates' lane unless a join
        has followed the lists already. """
        plan, sp = self.plan, self.plan.sparse
        if form == 'lists_after':
            # the layer that writes the logits: gpp_conv2d_igemm enqueues the deep lists behind its launch (gpp_conv_desc.lists_after) --
            # part of this op, on this stream, in front of the tower layers that read them
            d = self.desc(name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane)
            d.lists_after = sp.register_deep(sp.deep_desc(plan.cls_logits, plan.n_anchors, anchor_utils.NUM_BASE_ANCHORS, SCORE_THRESHOLD))
            reads, writes = list(src), list(out) + sp.deep_tensors()
            if sp.tower0_rows is not None:
                # ... and, behind the lists, the regression slice of the towers' first layer on the radius-4 rows (towers_0_split): the
                # library's launches under this op, which so reads the P maps and writes the slice and layer 0's lists
                first, p_maps, slice_maps = self.tower0
                sp.register_tower0(first, d)
                reads, writes = reads + p_maps, writes + slice_maps + sp.tower0_tensors()
            plan.emit(OP_CONV, d, name, reads, writes, flops=C.conv_flops(d), lane=lane, join=join, io=(src, out, None))
            return
        if form == 'dense':
            self.conv(name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane, join=join)
            if sp is not None and join and not lane:
                sp.lists_joined = True
            return
        dense = self.desc(name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane)
        dense.guard, dense.guard_value = sp.flag.data_ptr(), 1
        plan.emit(OP_CONV, dense, name, list(src) + [sp.flag], out, flops=C.conv_flops(dense), lane=lane, join=join or not sp.lists_joined,
                  io=(src, out, None))
        sp.lists_joined = True
        rows = self.desc(name, src, out, 3, pad=(1, 1), out_f32=True, lane=lane)
        rows.gather_rows, rows.gather_counts, rows.split_k = sp.rows.data_ptr(), sp.counts.data_ptr(), 1
        rows.guard, rows.guard_value = sp.flag.data_ptr(), 0
        # (flops 0: Plan.flops stays the reference graph's algorithmic count, which the dense launch above carries)
        plan.emit(OP_CONV, rows, name, list(src) + [sp.rows, sp.counts, sp.flag], out, lane=lane, io=(src, out, None))
        sp.dense.append(dense)
        sp.gathered.append(rows)

    # ------------------------------------------------------------------ behind the decode
    def poll(self):
        """ ground-plane polling (FitRoadPlanes) of the detections """
        plan, B, n_planes, torch, dev, D = self.plan, self.B, self.n_planes, self.torch, self.device, MAX_DETECTIONS
        plan.keypoints = torch.empty((B, D, 4, 3), dtype=torch.float32, device=dev)
        plan.keyplanes = torch.empty((B, D, 1, 4), dtype=torch.float32, device=dev)
        plan.residuals = torch.empty((B, D), dtype=torch.float32, device=dev)
        plan.best_index = torch.empty((B, D), dtype=torch.int32, device=dev)
        need = hip.c_size_t(0)
        hip.check(hip.lib().gpp_poll_workspace_bytes(B, n_planes, int(self.planes_batched), need), 'gpp_poll_workspace_bytes')
        plan.poll_ws = torch.empty((max(int(need.value), 16),), dtype=torch.uint8, device=dev)
        pd = PollDesc(plan.boxes.data_ptr(), plan.dimensions.data_ptr(), plan.orientations.data_ptr(), plan.P_inv.data_ptr(),
                      plan.planes.data_ptr(), plan.keypoints.data_ptr(), plan.keyplanes.data_ptr(), plan.residuals.data_ptr(),
                      plan.best_index.data_ptr(), plan.poll_ws.data_ptr(), plan.poll_ws.numel(), B, D, n_planes,
                      int(self.planes_batched), POLL_THRESHOLD, 0)
        plan.emit(OP_POLL, pd, 'fit_road_planes', [plan.boxes, plan.dimensions, plan.orientations, plan.P_inv, plan.planes],
                  [plan.keypoints, plan.keyplanes, plan.residuals, plan.best_index, plan.poll_ws], tag=2,    # tag 2: bench.py times it live too
                  flops=162.0 * B * D * n_planes)

    def pose(self):
        """ 6-DoF pose + KITTI fields of the detections (what bin/run_network.py does on the host after predict_on_batch), on lane 0
        behind the polling.  Rows, range-event snapshot and counts share ONE flat buffer, so that one copy brings a call's result to
        the host: [B x D x 36 rows | 2 words: the plan's range counter as the stream saw it | B counts (int32 bits)]. """
        plan, B, torch, dev, D = self.plan, self.B, self.torch, self.device, MAX_DETECTIONS
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

    def cuboid_nms(self):
        """ cuboid_nms=(metric, threshold): the greedy NMS of the cuboids (gpp_cuboid_nms_f64) on lane 0 behind the pose op, in place on
        its rows and counts; plan.pose_suppressor (B, D) int32 names the kept row that removed each suppressed one """
        plan, B, D = self.plan, self.B, MAX_DETECTIONS
        metric, threshold = self.model.cuboid_nms
        plan.pose_suppressor = self.torch.full((B, D), -1, dtype=self.torch.int32, device=self.device)
        nd = CuboidNmsDesc(plan.pose_rows.data_ptr(), plan.pose_counts.data_ptr(), plan.pose_suppressor.data_ptr(), threshold, B, D,
                           cuboid_nms_utils.metric_code(metric), 0)
        plan.emit(OP_CUBOID_NMS, nd, 'suppress_cuboids', [plan.pose_rows], [plan.pose_rows, plan.pose_counts, plan.pose_suppressor])

    def audit(self):
        """ range_audit=True: one gpp_channel_absmax launch behind every launch that writes (a part, a level or a channel slice of) a map
        that some convolution of the plan reads as its activation operand or adds as its residual -- the maps an x3 loop splits into
        (hi, lo) halves or reads pre-split -- on that launch's lane, into the map's row of plan.audit_table; the first op of the plan
        clears the table on the stream.  A map is a channel range of a buffer as its READERS name it (the three towers read three
        slices of the fused first layer's 896 channels: three maps; the five levels of a pyramid tensor: one map).  Placed once every
        op is known: who reads what is only known then.  Operands that never exist in HBM go to plan.audit_unobserved. """
        plan, torch, esz = self.plan, self.torch, self.model.esz
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

    def bind_workspaces(self):
        """ split-K partial tiles of the deep-K layers with a tiny per-image grid (res5 branch2b, P5..P7): one workspace per stream lane
        (concurrent launches must not share partial tiles), sized from the descriptors of the whole plan """
        plan = self.plan
        plan.workspaces = {lane: self.torch.empty((max(need, 16),), dtype=self.torch.uint8, device=self.device)
                           for lane, need in plan.ws_need.items()}
        for d, lane in plan.conv_descs:
            d.partial = plan.workspaces[lane].data_ptr()
            d.partial_bytes = plan.workspaces[lane].numel()
