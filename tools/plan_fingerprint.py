#!/usr/bin/env python3
"""
A hash of every plan of the CPU plan matrix (tests/helpers.plan_matrix), one line per configuration:

    python tools/plan_fingerprint.py > before.txt      # on the parent commit
    python tools/plan_fingerprint.py > after.txt       # on the change
    diff before.txt after.txt                          # empty: the change left every plan as it was

No GPU is needed: the model is built on the CPU device (hip.require_device patched, GPP_AUTOTUNE=0), and what the plan builder asks of the
library (FLOPs, workspace sizes, the split rule, the version) is host code.  The hash covers the canonical form of the plan: the ops in order,
each with its kind word as gpp_plan_run sees it (lane, join, sync and stage bits included), tag, name, FLOPs and every descriptor field,
recursively -- a pointer to another descriptor of the plan is replaced by that descriptor's own dump, a pointer into a torch tensor the plan or
the model holds by (the ordinal of that tensor's storage in order of first reference, byte offset) -- then the side lanes, the decode overlap,
the tagged ops, the anchor count and the feature maps of plan.io_parts / plan.features.  The form does not depend on where or in which order
the buffers were allocated.  A pointer that resolves to nothing is counted (`unresolved=`); it should be 0.

--verbose prints the canonical form instead of its hash (to see where two trees differ).
"""

import argparse
import bisect
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'ground-plane-polling_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from keras_retinanet_3D import models  # noqa: E402
from keras_retinanet_3D.backend import hip  # noqa: E402
from keras_retinanet_3D.layers import conv as C  # noqa: E402
from keras_retinanet_3D.models import weights as W  # noqa: E402
from tests import helpers  # noqa: E402


class Canon(object):
    """ the canonical form of one plan (see the module docstring) """

    def __init__(self, plan, model):
        self.descs = {ctypes.addressof(d): d for d in plan.keep if isinstance(d, ctypes.Structure)}
        spans, seen = {}, set()

        def collect(obj):
            if id(obj) in seen:
                return
            seen.add(id(obj))
            if isinstance(obj, torch.Tensor):
                s = obj.untyped_storage()
                if s.nbytes():
                    spans[s.data_ptr()] = s.data_ptr() + s.nbytes()
            elif isinstance(obj, dict):
                for v in obj.values():
                    collect(v)
            elif isinstance(obj, (list, tuple)):
                for v in obj:
                    collect(v)
            elif isinstance(obj, C.FMap):
                collect(obj.buf)
            elif type(obj).__name__ == 'Plan':
                collect(obj.__dict__)

        collect(plan.__dict__)
        collect(model.__dict__)
        collect(C._ZERO_PAGES)
        self.starts = sorted(spans)
        self.ends = [spans[s] for s in self.starts]
        self.ordinal = {}
        self.unresolved = 0

    def ptr(self, p):
        if not p:
            return 0
        if p in self.descs:
            return ('desc', self.dump(self.descs[p]))
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0 and p < self.ends[i]:
            s = self.starts[i]
            return ('buf', self.ordinal.setdefault(s, len(self.ordinal)), p - s)
        self.unresolved += 1
        return ('?',)

    def value(self, ctype, v):
        if ctype is ctypes.c_void_p:
            return self.ptr(v)
        if isinstance(v, ctypes.Structure):
            return self.dump(v)
        if isinstance(v, ctypes.Array):
            return [self.value(ctype._type_, x) for x in v]
        return repr(v) if isinstance(v, float) else v

    def dump(self, s):
        return [type(s).__name__] + [(name, self.value(ctype, getattr(s, name))) for name, ctype in s._fields_]

    def fmap(self, f):
        if f is None:
            return None
        return (self.ptr(f.buf.data_ptr()), f.off, f.B, f.H, f.W, f.C, f.pitch, f.bstride, f.split, f.half if f.split else None)

    def plan(self, plan):
        ops = [(plan.array[i].kind, tag, name, repr(flops), self.dump(desc)) for i, (_, tag, desc, name, flops) in enumerate(plan.ops)]
        io = [(name, [[[self.fmap(f) for f in fs or []] for fs in part] for part in parts]) for name, parts in plan.io_parts.items()]
        feats = [(k, self.fmap(v)) for k, v in sorted(plan.features.items())]
        extra = (sorted(plan.side_lanes.items()), plan.decode_overlap, plan.tagged, plan.n_anchors, self.fmap(plan.stem_out),
                 self.fmap(plan.pool_out), [self.fmap(f) for f in plan.relu_io])
        return [ops, io, feats, extra]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--verbose', action='store_true', help='print the canonical form of every plan instead of its hash')
    args = ap.parse_args()
    for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
        del os.environ[k]
    os.environ['GPP_AUTOTUNE'] = '0'
    hip.require_device = lambda: torch.device('cpu')
    weights, built = {}, {}
    for cfg in helpers.plan_matrix():
        bb, dt, kw, env, B, H, Wd = cfg
        kw = dict(kw)
        ragged = kw.pop('ragged', False)
        key = (bb, dt, tuple(sorted(kw.items())))
        if key not in built:
            if bb not in weights:
                weights[bb] = W.synthetic_weights(bb, 1234)
            built[key] = models.load_model(weights[bb], backbone_name=bb, dtype=dt, **kw)
        model = built[key]
        model._plans.clear()
        os.environ.update(env)
        try:
            plan = model.plan_for(B, H, Wd, 100, True, ragged=ragged)
        finally:
            for k in env:
                del os.environ[k]
        canon = Canon(plan, model)
        form = repr(canon.plan(plan))
        model._plans.clear()
        if args.verbose:
            print(helpers.plan_label(cfg))
            print(form)
        else:
            print('{}  {}  ops={} unresolved={}'.format(helpers.plan_label(cfg), hashlib.sha1(form.encode()).hexdigest()[:16], len(plan.ops),
                                                         canon.unresolved))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
