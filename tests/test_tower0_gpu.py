"""
Layer 0 of the regression tower on the 9 x 9 candidate set: the regression slice of pyramid_towers_0 as a layer of
both forms that the library enqueues behind the layer that writes the logits (gpp_conv_desc.conv_after, gpp_conv2d_deferred_register).

  * kernel level -- one 3 x 3, 512 -> 512 f16x3 layer registered as a deferred one behind a carrier: with the flag at 0 every listed row holds the
    bytes of the dense launch in both halves of the pre-split map and every other row keeps its poison, with the flag at 1 the whole map is the
    dense launch's; descriptors that break the rules are refused before anything is launched;
  * plan level at (2, 224, 352), the shape, frames and forced environment of tests/test_deep_tower_gpu.py -- GPP_SPARSE_TOWER_DEPTH 4 against 3
    and against 1: the same ops, FLOPs and lanes, the same bytes in every output, in the anchor and plane indices and in the head tensors read
    whole, the gathered launch doing the work; the dense path through the flag; an op run on its own writes its whole map.

Byte equality throughout: a gathered row IS the dense row (same K order, same epilogue), so there is no tolerance to state.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.layers import conv as C
from keras_retinanet_3D.utils import synthetic

pytestmark = pytest.mark.gpu

B = 2
LEVELS = [(9, 11), (5, 6)]
PIX = [h * w for h, w in LEVELS]
TOTAL = sum(PIX)
CIN = COUT = 512
AUTO = 8000256
POISON = 0x7fc0dead
BAD_ARG, UNSUPPORTED, ALIGN = -1, -4, -3
G = hip.GPP_MAX_GROUPS


class Layer(object):
    """ a tower layer over two levels (3 x 3, pad 1, ReLU, 512 -> 512, pre-split maps) as the deferred layer, and the same layer into a second
    buffer as its carrier; the dense result of both once """

    def __init__(self):
        dev = torch.device('cuda')
        g = torch.Generator().manual_seed(78)
        self.xbuf = torch.empty((B, TOTAL, CIN), dtype=torch.float32, device=dev)
        self.obuf = torch.empty((B, TOTAL, COUT), dtype=torch.float32, device=dev)
        self.cbuf = torch.empty((B, TOTAL, COUT), dtype=torch.float32, device=dev)
        self.ins, self.outs, self.carrier_outs, off = [], [], [], 0
        for h, w in LEVELS:
            fm = C.FMap(self.xbuf, B, h, w, CIN, off=off * CIN, bstride=TOTAL * CIN, split=True, half='f16x3')
            fm.write(torch.randn((B, h, w, CIN), generator=g))
            self.ins.append(fm)
            self.outs.append(C.FMap(self.obuf, B, h, w, COUT, off=off * COUT, bstride=TOTAL * COUT, split=True, half='f16x3'))
            self.carrier_outs.append(C.FMap(self.cbuf, B, h, w, COUT, off=off * COUT, bstride=TOTAL * COUT, split=True, half='f16x3'))
            off += h * w
        k = (torch.randn((3, 3, CIN, COUT), generator=g) * (2.0 / (9 * CIN)) ** 0.5).numpy()
        self.w = C.pack_weight(k, 'f16x3', dev)
        self.bias = (torch.randn((COUT,), generator=g) * 0.1).to(dev)
        self.scale = C.out_scale_of(k, dev)
        self.rows = torch.zeros((B * TOTAL,), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((G + 1,), dtype=torch.int32, device=dev)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.slot = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.poison()
        C.run_conv(self.desc(deep=False))
        C.run_conv(self.carrier())
        self.dense = self.bits()
        assert not (self.dense == POISON).any() and np.array_equal(self.bits(self.cbuf), self.dense)

    def desc(self, deep=True, deep_tile=0):
        d = C.conv_desc(self.ins, self.outs, self.w, self.bias, 3, 3, CIN, COUT, pad=(1, 1), relu=True, dtype='f16x3', out_scale=self.scale)
        d.range_counter = self.slot.data_ptr()
        if deep:
            d.deep_rows, d.deep_counts, d.deep_flag, d.deep_tile = self.rows.data_ptr(), self.counts.data_ptr(), self.flag.data_ptr(), deep_tile
        return d

    def carrier(self, handle=0):
        d = C.conv_desc(self.ins, self.carrier_outs, self.w, self.bias, 3, 3, CIN, COUT, pad=(1, 1), relu=True, dtype='f16x3', out_scale=self.scale)
        d.range_counter = self.slot.data_ptr()
        d.conv_after = handle
        return d

    def poison(self):
        self.obuf.view(torch.int32).fill_(POISON)
        self.cbuf.view(torch.int32).fill_(POISON)

    def bits(self, buf=None):
        return (self.obuf if buf is None else buf).view(torch.int32).cpu().numpy().copy()

    def put(self, lists):
        begin = 0
        rows = np.zeros((B * TOTAL,), np.int32)
        for p, lst in zip(PIX, lists):
            rows[begin:begin + len(lst)] = lst
            begin += B * p
        self.rows.copy_(torch.as_tensor(rows))
        self.counts.copy_(torch.as_tensor([len(x) for x in lists] + [0] * (G - len(lists)) + [sum(len(x) for x in lists)], dtype=torch.int32))

    def expected(self, lists):
        mask = np.zeros((B, TOTAL), bool)
        off = 0
        for p, lst in zip(PIX, lists):
            for m in lst:
                b, q = divmod(m, p)
                mask[b, off + q] = True
            off += p
        return np.where(mask[:, :, None], self.dense, np.int32(POISON))


@pytest.fixture(scope='module')
def layer():
    return Layer()


def register(desc):
    handle = ctypes.c_int32(0)
    rc = hip.lib().gpp_conv2d_deferred_register(ctypes.byref(desc), ctypes.byref(handle))
    return rc, handle.value


def run(desc):
    return hip.lib().gpp_conv2d_igemm(ctypes.byref(desc), hip.stream_ptr())


def test_a_deferred_layer_of_both_forms_behind_its_carrier(layer):
    L = layer
    rng = np.random.default_rng(5)
    cases = {'none': [[], []],
             'every row': [list(range(B * p)) for p in PIX],
             'random 70 %': [sorted(rng.choice(B * p, size=int(B * p * 0.7), replace=False).tolist()) for p in PIX],
             'one level empty': [[], sorted(rng.choice(B * PIX[1], size=17, replace=False).tolist())],
             'first and last row': [[0, B * PIX[0] - 1], [0, B * PIX[1] - 1]]}
    for tile in (0, AUTO):
        rc, handle = register(L.desc(deep_tile=tile))
        assert rc == 0 and handle > 0
        for name, lists in cases.items():
            L.put(lists)
            L.flag.fill_(0)
            L.poison()
            assert run(L.carrier(handle)) == 0
            got = L.bits()
            assert np.array_equal(got, L.expected(lists)), (name, tile, int((got != L.expected(lists)).sum()))
            assert np.array_equal(L.bits(L.cbuf), L.dense), name                  # the carrier's own launch is the dense one it always was
        L.flag.fill_(1)
        L.poison()
        assert run(L.carrier(handle)) == 0
        assert np.array_equal(L.bits(), L.dense) and np.array_equal(L.bits(L.cbuf), L.dense)
        # conv_before: in front of a plain dense reader the registered layer runs dense, whatever its lists and its flag say
        L.put(cases['first and last row'])
        L.flag.fill_(0)
        L.poison()
        d = L.carrier()
        d.conv_before = handle
        assert run(d) == 0
        assert np.array_equal(L.bits(), L.dense) and np.array_equal(L.bits(L.cbuf), L.dense)
        assert hip.lib().gpp_conv2d_deferred_release(handle) == 0
    torch.cuda.synchronize()


def test_descriptors_that_break_the_rules_are_refused_before_a_launch(layer):
    L = layer
    lib = hip.lib()
    L.put([[1, 2, 3], [4]])
    L.flag.fill_(0)
    L.poison()
    # what the library keeps: a valid layer of both forms on the deep lists that names nothing behind itself
    assert register(L.desc(deep=False)) == (BAD_ARG, 0)
    for fields, want in (({'deep_counts': None}, BAD_ARG), ({'deep_rows': L.rows.data_ptr() + 2}, ALIGN), ({'lists_after': 1}, BAD_ARG),
                         ({'conv_after': 1}, BAD_ARG), ({'conv_before': 1}, BAD_ARG), ({'C_out': 128}, UNSUPPORTED), ({'stride': 2}, UNSUPPORTED),
                         ({'guard': L.flag.data_ptr()}, BAD_ARG)):
        d = L.desc()
        for k, v in fields.items():
            setattr(d, k, v)
        rc, handle = register(d)
        assert rc == want and handle == 0, fields
    assert lib.gpp_conv2d_deferred_register(None, None) == BAD_ARG
    # the carrier: a handle nobody holds, a reserved word, or a carrier that is itself gathered, guarded or of both forms
    for handle in (-1, 1 << 30):
        assert run(L.carrier(handle)) == BAD_ARG
    rc, handle = register(L.desc())
    assert rc == 0 and lib.gpp_conv2d_deferred_run(handle, 1, None) == 0
    for fields in ({'conv_before': handle + 1}, {'conv_before': -1}, {'guard': L.flag.data_ptr()}, {'gather_rows': L.rows.data_ptr(), 'gather_counts': L.counts.data_ptr()},
                   {'deep_rows': L.rows.data_ptr(), 'deep_counts': L.counts.data_ptr(), 'deep_flag': L.flag.data_ptr()},
                   {'tower_rows': L.rows.data_ptr(), 'tower_counts': L.counts.data_ptr(), 'tower_flag': L.flag.data_ptr()}):
        d = L.carrier(handle)
        for k, v in fields.items():
            setattr(d, k, v)
        assert run(d) == BAD_ARG, fields
    assert lib.gpp_conv2d_deferred_release(handle) == 0
    assert run(L.carrier(handle)) == BAD_ARG and lib.gpp_conv2d_deferred_release(handle) == BAD_ARG
    assert lib.gpp_conv2d_deferred_run(0, 1, None) == BAD_ARG and lib.gpp_conv2d_deferred_run(-3, 0, None) == BAD_ARG
    torch.cuda.synchronize()
    assert (L.bits() == POISON).all() and (L.bits(L.cbuf) == POISON).all()         # nothing was launched


# ---------------------------------------------------------------------------------------------- plan level
SHAPE = (2, 224, 352)
TOWER0, CLS = 'pyramid_towers_0', 'pyramid_classification'


def run_model(env):
    env = dict({'GPP_AUTOTUNE': '0', 'GPP_SPARSE_TOWER_MIN_ROUNDS': '0', 'GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS': '0', 'GPP_CLS_LANE': '0'}, **env)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        batch, h, w = SHAPE
        rng = np.random.default_rng(0)
        img = rng.integers(0, 256, size=(batch, h, w, 3)).astype(np.float32) - np.array([103.939, 116.779, 123.68], np.float32)
        planes = synthetic.load_plane_database('100').astype(np.float32)
        _, P_inv = synthetic.synthetic_calibration()
        model = models.load_model('synthetic:1234', backbone_name='resnet50', dtype='f16x3')
        outs = model.predict_on_batch([img, np.tile(P_inv[None].astype(np.float32), (batch, 1, 1)), np.tile(planes[None], (batch, 1, 1))])
        plan = model.plan_for(batch, h, w, planes.shape[0], True)
        sp = plan.sparse
        names = [op[3] for op in plan.ops]
        state = {'deep_layers': sp.deep_layers, 'tower0': sp.tower0 is not None, 'rows': int(sp.rows.numel())}
        if sp.deep_layers:
            state.update(deep_totals=[int(c[G].item()) for c in sp.deep_counts], deep_flags=[int(f.item()) for f in sp.deep_flags],
                         deep_max_rows=sp.deep_max_rows)
        if sp.tower0 is not None:
            state.update(total0=int(sp.tower0_counts[G].item()), flag0=int(sp.tower0_flag.item()), stats0=int(sp.tower0_stats.item()),
                         conv_after=int(plan.ops[names.index(CLS)][2].conv_after), handle=sp.tower0_handle,
                         slice_cout=int(sp.tower0.C_out), rest_cout=int(plan.ops[names.index(TOWER0)][2].C_out))
        events = model.x3_range_events()
        outs = outs + [plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy()]
        heads = [plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy(), plan.cls_logits.cpu().numpy()]
        result = {'outs': outs, 'heads': heads, 'events': events, 'events_after_completion': model.x3_range_events(), 'state': state,
                  'names': names, 'op_flops': [op[4] for op in plan.ops], 'flops': plan.flops, 'lanes': list(plan.lanes),
                  'ordering': plan.check_stream_ordering()}
        # an op run on its own writes its whole map: pyramid_towers_0 over a poisoned map, every channel of every pixel
        wide = plan.io[TOWER0][1][0].buf
        assert wide.shape[2] == 896
        wide.view(torch.int32).fill_(POISON)
        model.run_op(plan, names.index(TOWER0))
        result['towers_0'] = wide.view(torch.int32).cpu().numpy().copy()
        if sp.tower0 is not None:
            model.run_op(plan, names.index(CLS))
            result['flags_behind_run_op'] = [int(f.item()) for f in sp.deep_flags] + [int(sp.tower0_flag.item())]
        return result
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def reference_run(depth):
    if depth not in _RUNS:
        _RUNS[depth] = got = run_model({'GPP_SPARSE_TOWER_DEPTH': str(depth)})
        assert not got['state']['tower0'] and got['state']['deep_layers'] == min(2, depth - 1) and (got['outs'][2] > 0.05).sum() > 0
        assert not (got['towers_0'] == POISON).any()
    return _RUNS[depth]


def same_plan_and_bytes(got, want):
    assert got['ordering'] == [] and got['names'] == want['names'] and got['op_flops'] == want['op_flops'] and got['flops'] == want['flops']
    assert got['lanes'] == want['lanes']
    for a, b in zip(got['outs'] + got['heads'], want['outs'] + want['heads']):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert got['events'] == got['events_after_completion']            # reading the head tensors whole counts no event a second time
    assert not (got['towers_0'] == POISON).any() and np.array_equal(got['towers_0'], want['towers_0'])


def test_depth_4_gives_the_plan_and_the_bytes_of_depth_3_and_of_depth_1():
    got = run_model({'GPP_SPARSE_TOWER_DEPTH': '4'})
    st = got['state']
    assert st['tower0'] and st['deep_layers'] == 2 and st['slice_cout'] == 512 and st['rest_cout'] == 384
    assert st['handle'] > 0 and st['conv_after'] == st['handle']
    # the gathered launch did the work, on at least layer 1's rows and on fewer than all: neither an empty nor a dense run
    assert st['flag0'] == 0 and st['stats0'] == 0 and st['deep_flags'] == [0, 0]
    assert 0 < st['deep_totals'][1] <= st['total0'] <= st['deep_max_rows'] < st['rows']
    assert got['flags_behind_run_op'] == [1, 1, 1]
    same_plan_and_bytes(got, reference_run(3))
    same_plan_and_bytes(got, reference_run(1))


def test_the_dense_path_of_layer_0_gives_the_same_bytes():
    """ largest deep share 0: every step sets flag0 with the other two, the slice's dense launch runs and its gathered one returns at once """
    got = run_model({'GPP_SPARSE_TOWER_DEPTH': '4', 'GPP_SPARSE_TOWER_DEEP_MAX_SHARE': '0'})
    st = got['state']
    assert st['tower0'] and st['deep_max_rows'] == 0 and st['flag0'] == 1 and st['deep_flags'] == [1, 1] and st['total0'] > 0
    same_plan_and_bytes(got, reference_run(3))
