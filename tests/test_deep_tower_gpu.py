"""
Deep sparse regression tower: layers 1 and 2 of the regression tower on the 7 x 7 and 5 x 5 neighbourhoods of the
candidates' pixels, from lists made on the caller's stream behind pyramid_classification.

  * kernel level -- one 3 x 3, 512 -> 512 f16x3 op with gpp_conv_desc.deep_rows / deep_counts / deep_flag: with the flag at 0 every listed row
    holds the bytes of the dense launch in both halves of the split map and no other byte is written, with the flag at 1 the whole map is the
    dense launch's; the fields are validated as the tower_* fields are;
  * plan level at (2, 224, 352) -- GPP_SPARSE_TOWER_DEPTH 3 and 2 against 1 and against GPP_SPARSE_TOWER=0: the same bytes in every output and
    in the head tensors read whole, the same ops, the same range events.

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
AUTO = 8000256                                                    # include/gpp.h: the height chosen on the device
POISON = 0x7fc0dead
BAD_ARG, UNSUPPORTED = -1, -4


class Layer(object):
    """ one tower layer over the two levels: 3 x 3, pad 1, ReLU, 512 -> 512, pre-split input and output maps; the dense result once """

    def __init__(self):
        dev = torch.device('cuda')
        g = torch.Generator().manual_seed(77)
        self.xbuf = torch.empty((B, TOTAL, CIN), dtype=torch.float32, device=dev)
        self.obuf = torch.empty((B, TOTAL, COUT), dtype=torch.float32, device=dev)
        self.ins, self.outs, off = [], [], 0
        for h, w in LEVELS:
            fm = C.FMap(self.xbuf, B, h, w, CIN, off=off * CIN, bstride=TOTAL * CIN, split=True, half='f16x3')
            fm.write(torch.randn((B, h, w, CIN), generator=g))
            self.ins.append(fm)
            self.outs.append(C.FMap(self.obuf, B, h, w, COUT, off=off * COUT, bstride=TOTAL * COUT, split=True, half='f16x3'))
            off += h * w
        k = (torch.randn((3, 3, CIN, COUT), generator=g) * (2.0 / (9 * CIN)) ** 0.5).numpy()
        self.w = C.pack_weight(k, 'f16x3', dev)
        self.bias = (torch.randn((COUT,), generator=g) * 0.1).to(dev)
        self.scale = C.out_scale_of(k, dev)
        self.rows = torch.zeros((B * TOTAL,), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((hip.GPP_MAX_GROUPS + 1,), dtype=torch.int32, device=dev)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.slot = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.poison()
        C.run_conv(self.desc(deep=False))
        self.dense = self.bits()
        assert not (self.dense == POISON).any()

    def desc(self, deep=True, deep_tile=0):
        d = C.conv_desc(self.ins, self.outs, self.w, self.bias, 3, 3, CIN, COUT, pad=(1, 1), relu=True, dtype='f16x3', out_scale=self.scale)
        d.range_counter = self.slot.data_ptr()
        if deep:
            d.deep_rows, d.deep_counts, d.deep_flag, d.deep_tile = self.rows.data_ptr(), self.counts.data_ptr(), self.flag.data_ptr(), deep_tile
        return d

    def poison(self):
        self.obuf.view(torch.int32).fill_(POISON)

    def bits(self):
        return self.obuf.view(torch.int32).cpu().numpy().copy()          # (B, TOTAL, C_out): both halves of every 32-channel block

    def put(self, lists):
        begin = 0
        rows = np.zeros((B * TOTAL,), np.int32)
        for p, lst in zip(PIX, lists):
            rows[begin:begin + len(lst)] = lst
            begin += B * p
        self.rows.copy_(torch.as_tensor(rows))
        self.counts.copy_(torch.as_tensor([len(x) for x in lists] + [0] * (hip.GPP_MAX_GROUPS - len(lists)) + [sum(len(x) for x in lists)],
                                          dtype=torch.int32))

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


def run(desc):
    return hip.lib().gpp_conv2d_igemm(ctypes.byref(desc), hip.stream_ptr())


def test_one_op_of_both_forms_on_the_deep_lists(layer):
    L = layer
    rng = np.random.default_rng(4)
    cases = {'none': [[], []],
             'every row': [list(range(B * p)) for p in PIX],
             'random 60 %': [sorted(rng.choice(B * p, size=int(B * p * 0.6), replace=False).tolist()) for p in PIX],
             'one level empty': [sorted(rng.choice(B * PIX[0], size=70, replace=False).tolist()), []],
             'first and last row': [[0, B * PIX[0] - 1], [0, B * PIX[1] - 1]]}
    for name, lists in cases.items():
        L.put(lists)
        for tile in (0, AUTO, 8128256):
            L.flag.fill_(0)
            L.poison()
            C.run_conv(L.desc(deep_tile=tile))
            got = L.bits()
            assert np.array_equal(got, L.expected(lists)), (name, tile, int((got != L.expected(lists)).sum()))
        L.flag.fill_(1)
        L.poison()
        C.run_conv(L.desc())
        assert np.array_equal(L.bits(), L.dense), name
    # any other value of the flag: neither launch works
    L.flag.fill_(2)
    L.poison()
    C.run_conv(L.desc())
    assert (L.bits() == POISON).all()


def test_the_deep_fields_are_validated_as_the_tower_fields_are(layer):
    L = layer
    L.put([[1, 2, 3], [4]])
    L.flag.fill_(0)

    def both(**fields):
        d = L.desc()
        for k, val in fields.items():
            setattr(d, k, val)
        return run(d)
    assert both() == 0
    assert both(deep_counts=None) == BAD_ARG and both(deep_flag=None) == BAD_ARG and both(deep_rows=None) == BAD_ARG
    assert both(gather_rows=L.rows.data_ptr(), gather_counts=L.counts.data_ptr()) == BAD_ARG
    assert both(guard=L.flag.data_ptr()) == BAD_ARG
    assert both(tower_rows=L.rows.data_ptr(), tower_counts=L.counts.data_ptr(), tower_flag=L.flag.data_ptr()) == BAD_ARG      # never both sets
    assert both(deep_tile=1256256) == BAD_ARG and both(deep_tile=6064064) == UNSUPPORTED
    assert both(deep_rows=L.rows.data_ptr() + 2) == -3                             # GPP_ERR_ALIGN
    assert both(stride=2) == UNSUPPORTED and both(split_k=3) == UNSUPPORTED and both(C_out=128) == UNSUPPORTED
    assert both(x3_split=1) == UNSUPPORTED and both(x3_split=2) == UNSUPPORTED
    d = L.desc(deep=False)
    d.deep_tile = AUTO
    assert run(d) == BAD_ARG                                                       # a deep tile without the lists
    # lists_after: a handle nobody holds is refused before anything is launched
    L.poison()
    for handle in (-1, 1 << 30):
        d = L.desc(deep=False)
        d.lists_after = handle
        assert run(d) == BAD_ARG
    assert (L.bits() == POISON).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- plan level
SHAPE = (2, 224, 352)
G = hip.GPP_MAX_GROUPS


def run_model(env):
    # (GPP_CLS_LANE=0: at B <= 2 the classification tower runs on a side lane by default, and such a plan does not take the form -- the rule
    # of tests/test_deep_tower_cpu.py; every run here, the references too, is the plan a batch of 8 gets)
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
        state = {'deep_layers': sp.deep_layers if sp is not None else 0}
        if sp is not None and sp.tower_rows is not None:
            state.update(tower_total=int(sp.tower_counts[G].item()), tower_flag=int(sp.tower_flag.item()), listed=int(sp.counts[G].item()))
        if state['deep_layers']:
            state.update(deep_totals=[int(c[G].item()) for c in sp.deep_counts], deep_flags=[int(f.item()) for f in sp.deep_flags],
                         stats=sp.deep_stats.cpu().numpy().tolist(), deep_max_rows=sp.deep_max_rows)
        events = model.x3_range_events()
        outs = outs + [plan.anchor_index.cpu().numpy(), plan.best_index.cpu().numpy()]
        heads = [plan.regression.cpu().numpy(), plan.regression_dim.cpu().numpy(), plan.cls_logits.cpu().numpy()]
        result = {'outs': outs, 'heads': heads, 'events': events, 'events_after_completion': model.x3_range_events(), 'state': state,
                  'names': [op[3] for op in plan.ops], 'op_flops': [op[4] for op in plan.ops], 'flops': plan.flops,
                  'ordering': plan.check_stream_ordering(),
                  'deep': [op[3] for op in plan.ops if op[0] == 3 and op[2].deep_rows]}
        if state['deep_layers']:
            # an op run on its own writes its whole map: behind pyramid_classification alone both flags read 1
            model.run_op(plan, result['names'].index('pyramid_classification'))
            result['flags_behind_run_op'] = [int(f.item()) for f in sp.deep_flags]
        return result
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def reference_run(name):
    if name not in _RUNS:
        _RUNS[name] = run_model({'depth 1': {'GPP_SPARSE_TOWER_DEPTH': '1'}, 'dense tower': {'GPP_SPARSE_TOWER': '0'}}[name])
        got = _RUNS[name]
        assert got['deep'] == [] and got['state']['deep_layers'] == 0 and (got['outs'][2] > 0.05).sum() > 0
        assert ('tower_total' in got['state']) == (name == 'depth 1')
    return _RUNS[name]


def same_bytes(got, want):
    assert got['ordering'] == [] and got['names'] == want['names'] and got['op_flops'] == want['op_flops'] and got['flops'] == want['flops']
    for a, b in zip(got['outs'] + got['heads'], want['outs'] + want['heads']):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert got['events'] == got['events_after_completion']            # reading the head tensors whole counts no event a second time


@pytest.mark.parametrize('depth', [3, 2])
def test_deep_plans_give_the_bytes_of_depth_1_and_of_the_dense_tower(depth):
    got = run_model({'GPP_SPARSE_TOWER_DEPTH': str(depth)})
    st = got['state']
    assert got['deep'] == ['pyramid_regression_1', 'pyramid_regression_2'][3 - depth:] and st['deep_layers'] == depth - 1
    assert st['deep_flags'] == [0] * (depth - 1) and st['tower_flag'] == 0          # the gathered launches did the work ...
    totals = st['deep_totals']                                                   # ... layer 2 on at least layer 3's rows, layer 1 on at least layer 2's
    assert st['tower_total'] <= totals[0] <= st['deep_max_rows'] and (depth == 2 or totals[0] <= totals[1] <= st['deep_max_rows'])
    assert st['stats'][:3] == [st['listed'], st['tower_total'], 0]                  # the marks are the candidates' pixels, their dilation the tower's rows
    assert got['flags_behind_run_op'] == [1] * (depth - 1)
    same_bytes(got, reference_run('depth 1'))
    same_bytes(got, reference_run('dense tower'))


def test_the_dense_path_of_a_deep_plan_gives_the_same_bytes():
    """ largest deep share 0: every step sets both deep flags, the dense launches run and the gathered ones return at once; layer 3 stays gathered """
    got = run_model({'GPP_SPARSE_TOWER_DEEP_MAX_SHARE': '0'})
    st = got['state']
    assert st['deep_layers'] == 2 and st['deep_max_rows'] == 0 and st['deep_flags'] == [1, 1] and st['tower_flag'] == 0 and st['deep_totals'][0] > 0
    same_bytes(got, reference_run('depth 1'))


def test_a_dense_reader_makes_every_layer_in_front_of_it_dense():
    """ the tower's share 0 and the deep share 1: layer 3 runs dense, so layers 2 and 1 do -- whatever their own limit allows """
    got = run_model({'GPP_SPARSE_TOWER_MAX_SHARE': '0', 'GPP_SPARSE_TOWER_DEEP_MAX_SHARE': '1'})
    st = got['state']
    assert st['deep_layers'] == 2 and st['tower_flag'] == 1 and st['stats'][2] == 1 and st['deep_flags'] == [1, 1]
    assert max(st['deep_totals']) <= st['deep_max_rows']
    same_bytes(got, reference_run('depth 1'))
