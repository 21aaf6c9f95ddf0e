"""
Per-layer tile selection: autotune(model, plan) times the candidate tiles of every layer of a plan on the device and writes the fastest
into its descriptor; TuneCache remembers the choices per (layer, batch, image size) and keeps them in a JSON file (GPP_TUNE_CACHE).
A tile NEVER changes a result (same K order per output element, test_every_tile_gives_identical_results), so ranks and plans may choose
differently without any effect on the outputs; split-K, which would, is not tuned (gpp_conv2d_split_rule).
"""

import ctypes
import json
import os

from ..backend import hip
from ..layers import conv as C
from .plan import DETECT_OPS, OP_CONV, OP_CONV_PREACT, OP_MOBILENET_BLOCK, OP_POLL, OP_TAIL, TOWER0, PlanOp


class TuneCache(object):
    """ the tile choices of one model, (layer, B, H, W) -> (tile, us), and their file: one JSON object for every model that names it,
    key 'cfg|backbone|dtype|layer|B|H|W' -> [tile, us].  config: what a choice is valid for besides the rest of its key -- the build of
    the library (tile codes come and go with it: gpp_version() carries a hash of the kernel sources) and the plan options that change
    which maps are pre-split or fused (PlanOptions.tune_key, the same at every batch): a tile timed on a float32 map may not even exist
    for the pre-split form of the same layer.  Worked out once, when the model makes its cache (for_model). """

    def __init__(self, config, backbone, dtype):
        self.config, self.backbone, self.dtype = config, backbone, dtype
        self.entries = {}

    @classmethod
    def for_model(cls, model):
        ver = hip.lib().gpp_version().decode().split('src:')[-1]
        return cls('v2;{};{}'.format(ver, model._plan_options(1).tune_key), model.backbone_name, model.dtype)

    def get(self, key):
        return self.entries.get(key)

    def put(self, key, value):
        self.entries[key] = value

    def drop(self, key):
        del self.entries[key]

    def load(self, path):
        """ the entries of the file that are this model's: same configuration, backbone and type """
        if not path or not os.path.exists(path):
            return
        with open(path) as f:
            for key, val in json.load(f).items():
                parts = key.split('|')
                if len(parts) != 7:              # (files of rounds 1-3: no library hash in the key -- ignored, the layers are timed again)
                    continue
                cfg, bb, dt, name, b, h, w = parts
                if (cfg, bb, dt) == (self.config, self.backbone, self.dtype):
                    self.put((name, int(b), int(h), int(w)), (int(val[0]), float(val[-1])))

    def save(self, path):
        """ this model's entries into the file, beside whatever else it holds (a file that does not parse counts as empty).  Rank 0 only,
        through a temporary file + os.replace: readers never see a torn file, ranks never race. """
        if not path or int(os.environ.get('RANK', '0')) != 0:
            return
        data = {}
        if os.path.exists(path):
            try:
                with open(path) as f:
                    data = json.load(f)
            except ValueError:
                data = {}
        for (name, b, h, w), val in self.entries.items():
            data['|'.join([self.config, self.backbone, self.dtype, name, str(b), str(h), str(w)])] = list(val)
        tmp = '{}.tmp.{}'.format(path, os.getpid())
        with open(tmp, 'w') as f:
            json.dump(data, f, indent=0, sort_keys=True)
        os.replace(tmp, path)


def candidates(query, desc, capacity):
    """ the tile codes one of the library's *_tile_candidates entry points lists for a descriptor, in its order (at most `capacity`) """
    tiles, count = (ctypes.c_int * capacity)(), ctypes.c_int(0)
    hip.check(query(ctypes.byref(desc), tiles, capacity, ctypes.byref(count)), query.__name__)
    return list(tiles[:min(count.value, capacity)])


def as_gathered(desc):
    """ a layer of both forms as the gathered launch it enqueues on its dilated lists: what the library lists tiles for """
    rows = type(desc).from_buffer_copy(desc)
    rows.gather_rows, rows.gather_counts = desc.tower_rows, desc.tower_counts
    rows.tower_rows = rows.tower_counts = rows.tower_flag = None
    rows.tower_tile, rows.split_k = 0, 1
    return rows


def tower_tiles(desc):
    """ the tiles the gathered launch of a layer of both forms may take: the library's candidates for the layer as a gathered one """
    return [t for t in candidates(hip.lib().gpp_conv2d_tile_candidates, as_gathered(desc), 32) if t]


def tile_choices(model, plan, index, kind, target):
    """ the tiles one op can take: the fused tail's row counts, the pre-activation conv's candidates, or the conv's candidates that its
    launcher accepts for this shape (a trial launch each: a candidate the launcher refuses is skipped, as the autotuner does) """
    lib = hip.lib()
    if kind == OP_TAIL:
        return (64, 96, 128, 160) if model.dtype in C.X3_TYPES else (96, 128, 160)
    if kind == OP_MOBILENET_BLOCK:
        return candidates(lib.gpp_mobilenet_block_tile_candidates, target, 16)
    if kind == OP_CONV_PREACT:
        return candidates(lib.gpp_conv2d_preact_tile_candidates, target, 16)
    ok = []
    for tile in candidates(lib.gpp_conv2d_tile_candidates, target, 32):
        target.tile_hint = tile
        if lib.gpp_plan_run(ctypes.byref(plan.array, index * ctypes.sizeof(PlanOp)), 1, hip.stream_ptr(), None, 0) == 0:
            ok.append(tile)
    return ok


def fastest(model, plan, index, desc, field, choices, iters):
    """ (choice, us) of the fastest value of desc.<field> for one op, timed here: per choice one warm-up launch, then `iters` launches
    between two events """
    torch, times = model.torch, {}
    for choice in choices:
        setattr(desc, field, choice)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        model.run_op(plan, index)
        e0.record()
        for _ in range(iters):
            model.run_op(plan, index)
        e1.record()
        e1.synchronize()
        times[choice] = e0.elapsed_time(e1) * 1000.0 / iters
    best = min(times, key=times.get)
    return best, round(times[best], 2)


def time_tiles(model, plan, index, kind, desc, target, flops):
    """ (tile, us) of the fastest choice of one op: the fused tail's row counts timed here (GPP_TAIL64=0: not 64), the conv tiles by
    the library -- fewer launches per candidate for the float32 path, whose launches are 3 x as long (round 4: the x3 types on those
    counts rested a big layer's choice on four launches per candidate, and one tuning run in ~60 picked a tile that cost 5 %) """
    if kind == OP_TAIL:
        rows = [r for r in tile_choices(model, plan, index, kind, target) if r != 64 or os.environ.get('GPP_TAIL64', '1') != '0']
        return fastest(model, plan, index, desc, 'tile_rows', rows, 16)
    lib, slow = hip.lib(), model.dtype == 'f32'
    iters = (2 if slow else 6) if flops > 5e10 else (4 if slow else 16)
    best = ctypes.c_float(0.0)
    if kind == OP_MOBILENET_BLOCK:
        hip.check(lib.gpp_mobilenet_block_autotune(ctypes.byref(target), iters, hip.stream_ptr(), ctypes.byref(best)), 'gpp_mobilenet_block_autotune')
    elif kind == OP_CONV_PREACT:
        hip.check(lib.gpp_conv2d_preact_autotune(ctypes.byref(target), desc.in_scale, desc.in_shift, iters, hip.stream_ptr(), ctypes.byref(best)),
                  'gpp_conv2d_preact_autotune')
    else:
        hip.check(lib.gpp_conv2d_autotune(ctypes.byref(target), iters, hip.stream_ptr(), ctypes.byref(best)), 'gpp_conv2d_autotune')
    return int(target.tile_hint), round(float(best.value), 2)


def time_tower_tiles(model, plan, index, desc):
    """ (tile, us) of the fastest gathered tile of a layer of both forms, on every third pixel; the flag is 1 again afterwards """
    sp = plan.sparse
    sp.put_every_nth(model.torch, 3, tower=True)
    sp.tower_flag.fill_(0)
    best = fastest(model, plan, index, desc, 'tower_tile', tower_tiles(desc), 8)
    sp.tower_flag.fill_(1)
    sp.tower_counts.zero_()
    return best


def autotune(model, plan):
    """ Choose the block tile of every conv layer of this plan by timing the candidates on the device
    (gpp_conv2d_autotune), layer by layer on realistic activations (a noise frame pushed through the layers
    before).  Whether a layer's tile grid fills the 256 CUs in 1.07 or 0.95 rounds decides its time by up to 1.5x
    and is cheap to measure.  Choices are remembered per (layer, batch, image size) in the model's TuneCache and can be
    persisted with GPP_TUNE_CACHE=<file.json>.  GPP_AUTOTUNE=0 keeps the library heuristic.
    The fused tails choose their row count (tile_rows), DenseNet's pre-activation convs the tile of their inner conv, MobileNet's
    blocks their own tile_hint. """
    model._require_hip()
    cache, lib = model._tune, hip.lib()
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
                plan.sparse.put_every_nth(model.torch)
                name = name + '@rows'
        if kind == OP_CONV and name == TOWER0 and plan.sparse is not None and plan.sparse.tower0 is not None:
            # the launch under this name computes the columns behind the regression slice only (PlanBuilder.towers_0_split): another layer
            # than the fused one, timed under a key of its own -- the fused layer's key keeps its meaning
            name = name + '@cols'
        model.run_op(plan, index)
        if kind not in (OP_CONV, OP_TAIL, OP_CONV_PREACT, OP_MOBILENET_BLOCK):
            continue
        # where the choice is written: the conv's own descriptor, the pre-activation's inner one, the tail's row count
        target = plan.inner[id(desc)][0] if kind == OP_CONV_PREACT else desc
        field = 'tile_rows' if kind == OP_TAIL else 'tile_hint'
        if rnd is not None:
            setattr(target, field, rnd.choice(tile_choices(model, plan, index, kind, target)))
            plan.tuning[name] = (int(getattr(target, field)), 0.0)
            model.run_op(plan, index)
            continue
        key = (name, target.B if kind == OP_MOBILENET_BLOCK else (plan.inner[id(desc)][0] if kind == OP_TAIL else target).batch, H, Wd)     # (a half-batch launch is tuned as what it is)
        if kind == OP_CONV and cache.get(key) and cache.get(key)[0] not in candidates(lib.gpp_conv2d_tile_candidates, desc, 64):
            cache.drop(key)                 # a remembered tile this build does not offer for this layer: time the layer again
        if cache.get(key) is None:
            cache.put(key, time_tiles(model, plan, index, kind, desc, target, flops))
            fresh = True
        setattr(target, field, cache.get(key)[0])
        plan.tuning[name] = cache.get(key)
        plan.tuning_parts.setdefault(name, []).append(cache.get(key))
        if kind == OP_CONV and desc.tower_rows:
            # a layer of both forms: the dense tile was timed above (the lists' flag is 1 outside a run); the gathered tiles on a synthetic
            # list of every THIRD pixel -- between what real frames list and the crossover -- with the flag clear
            rows_key = (name + '@rows',) + key[1:]
            if cache.get(rows_key) and cache.get(rows_key)[0] not in tower_tiles(desc):
                cache.drop(rows_key)
            if cache.get(rows_key) is None:
                cache.put(rows_key, time_tower_tiles(model, plan, index, desc))
                fresh = True
            desc.tower_tile = cache.get(rows_key)[0]
            plan.tuning[name + '@rows'] = cache.get(rows_key)
    if plan.sparse is not None:
        for d in plan.sparse.deep:           # the same layer shape as the last layer: the tile its gathered launches were timed to
            d.deep_tile = plan.sparse.tower[0].tower_tile
        if plan.sparse.tower0 is not None:
            # layer 0's regression slice has layer 1's shape: its dense tile and the gathered one; the library holds a copy of the descriptor
            plan.sparse.tower0.tile_hint = plan.sparse.deep[0].tile_hint
            plan.sparse.tower0.deep_tile = plan.sparse.tower[0].tower_tile
            plan.sparse.register_tower0()
        plan.sparse.reset(model.torch)
    model.torch.cuda.synchronize()
    if fresh:
        cache.save(os.environ.get('GPP_TUNE_CACHE'))
