"""
The HIP decode on the constructed cases of tests/decode_cases.py: every branch of nms_kernel's sort, histogram pre-selection, on-chip and
global-memory NMS and guard-banded overlap test, the orientation_specific_filter twins, non-finite logits, a reused workspace, the
separately enqueued stages and the refusals of the C ABI, against oracle/decode_np.py.  Bar: the five outputs bit for bit
(helpers.bits_equal), the anchor indices and the candidate counts exact.  No tolerance is involved.

tests/test_decode_selection_cpu.py shows, on the oracle alone, that each case reaches the branch it is named for.
"""
import ctypes

import numpy as np
import pytest

import helpers
import decode_cases as dc
from keras_retinanet_3D.layers.filter_detections import FilterDetections, filter_detections

pytestmark = pytest.mark.gpu

OUTPUTS = ('boxes', 'dimensions', 'scores', 'labels', 'orientations')


def compare(case, got, got_index, got_counts=None):
    """ got: the five outputs as NumPy arrays; every named claim first (a clearer message than an array's), then everything """
    ref, ref_idx = case.oracle()
    got_index = np.asarray(got_index).astype(np.int64)
    for c in case.claims:
        b, o = c['list']
        if o is None:
            kept = set(got_index[b][got_index[b] >= 0].tolist())
            assert set(c.get('has', ())) <= kept and not (set(c.get('lacks', ())) & kept), '{}: {}'.format(case.name, c)
    assert np.array_equal(got_index, ref_idx), case.name
    if got_counts is not None:
        assert np.array_equal(np.asarray(got_counts), case.candidate_counts()), case.name
    ref, got = [r.copy() for r in ref], [np.array(g) for g in got]
    for b, a in case.unpinned:                                 # box columns 6 and 10 of these rows: see decode_cases.case_nonfinite
        rows = np.flatnonzero(ref_idx[b] == a)
        assert rows.size
        for arr in (ref[0], got[0]):
            arr[b, rows, 6] = arr[b, rows, 10] = 0
    for g, r, key in zip(got, ref, OUTPUTS):
        assert g.dtype == r.dtype and helpers.bits_equal(g, r), '{}: {}'.format(case.name, key)


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('name', dc.NAMES)
def test_hip_decode_selection_case_against_oracle(name, fused):
    """ the selection reads the four corner regressions through either layout; the cases do not depend on it, so each runs in both """
    case = dc.get(name)
    reg = dc.to_fused(case.regression) if fused else case.regression.copy()
    out = filter_detections(case.logits.copy(), reg, case.regression_dim.copy(), case.anchors.copy(), fused_regression=fused, **case.kwargs)
    compare(case, out[:5], out[5], out[6])


def device_inputs(case, fused=False):
    import torch
    from keras_retinanet_3D.backend import hip
    dev = hip.require_device()
    reg = dc.to_fused(case.regression) if fused else case.regression
    return dev, [torch.as_tensor(np.array(a)).to(dev) for a in (case.logits, reg, case.regression_dim, case.anchors)]


def outputs_of(op):
    return [o.cpu().numpy() for o in (op.boxes, op.dimensions, op.scores, op.labels, op.orientations)]


def test_one_workspace_through_fallback_lds_empty_and_fallback_again():
    """ one FilterDetections instance: the first call leaves 8300 sorted keys, their zero padding, alive bytes and kept-key slots behind;
    a shorter list, an empty image and the first case again must not see any of it """
    seq = dc.workspace_sequence()
    dev, _ = device_inputs(seq[0])
    op = FilterDetections(1, seq[0].A, dev)
    for case in seq:
        _, args = device_inputs(case)
        op(*args)
        compare(case, outputs_of(op), op.anchor_index.cpu().numpy(), op.counts[:1].cpu().numpy())


@pytest.mark.parametrize('path', dc.PATHS)
def test_stages_enqueued_separately_on_each_path(path):
    """ gpp_detect_stages_f32(CANDIDATES), (SELECT), (EMIT) one after the other, one case per path of nms_kernel """
    from keras_retinanet_3D.backend import hip
    case = dc.get(dc.STAGED[path])
    dev, tensors = device_inputs(case, fused=True)
    op = FilterDetections(case.B, case.A, dev, fused_regression=True, **case.kwargs)
    for o in (op.boxes, op.dimensions, op.scores):
        o.fill_(float('nan'))
    args = op.args(*tensors) + (hip.stream_ptr(),)
    for stage in (1, 2, 4):
        hip.check(hip.lib().gpp_detect_stages_f32(stage, *args), 'gpp_detect_stages_f32')
    compare(case, outputs_of(op), op.anchor_index.cpu().numpy(), op.counts[:case.B].cpu().numpy())


def test_refusals_of_the_c_abi():
    """ what gpp_detect_f32 / gpp_detect_osf_f32 refuse, and with which code; B == 0 is accepted and touches nothing """
    import torch
    from keras_retinanet_3D.backend import hip
    lib, dev = hip.lib(), hip.require_device()
    OK, BAD_ARG, WORKSPACE, ALIGN, UNSUPPORTED = 0, -1, -2, -3, -4
    A, D = 24, 100

    def call(B=1, n_anchors=A, max_det=D, osf=False, logits_offset=0, short=0):
        f32, i32 = torch.float32, torch.int32
        rows = max(B, 1)
        logits = torch.full((rows * n_anchors * 8 + 4,), -9.0, dtype=f32, device=dev)
        reg = torch.zeros((rows * n_anchors * 12,), dtype=f32, device=dev)
        dim = torch.zeros((rows * n_anchors * 3,), dtype=f32, device=dev)
        anchors = torch.zeros((n_anchors * 4,), dtype=f32, device=dev)
        outs = [torch.full((rows * 128 * k,), 7.0, dtype=f32, device=dev) for k in (12, 3, 1)] + \
               [torch.full((rows * 128,), 7, dtype=i32, device=dev) for _ in range(3)] + [torch.full((rows,), 7, dtype=i32, device=dev)]
        need = hip.c_size_t(0)
        size_fn = lib.gpp_detect_osf_workspace_bytes if osf else lib.gpp_detect_workspace_bytes
        assert size_fn(max(B, 1), n_anchors, need) == OK
        ws = torch.empty((int(need.value),), dtype=torch.uint8, device=dev)
        fn = lib.gpp_detect_osf_f32 if osf else lib.gpp_detect_f32
        rc = fn(ctypes.c_void_p(logits.data_ptr() + logits_offset), hip.ptr(reg), hip.ptr(dim), hip.ptr(anchors), B, n_anchors, dc.NBA, 0, 0.05, 0.5, max_det,
                *([hip.ptr(o) for o in outs] + [hip.ptr(ws), int(need.value) - short, hip.stream_ptr()]))
        torch.cuda.synchronize()
        return rc, outs

    assert call()[0] == OK
    assert call(max_det=0)[0] == BAD_ARG and call(max_det=129)[0] == BAD_ARG
    assert call(max_det=128)[0] == OK
    assert call(B=64)[0] == OK and call(B=65)[0] == UNSUPPORTED
    assert call(B=16, osf=True)[0] == OK and call(B=17, osf=True)[0] == UNSUPPORTED
    assert call(n_anchors=A + 1)[0] == UNSUPPORTED and call(n_anchors=A - 1)[0] == UNSUPPORTED
    assert call(logits_offset=4)[0] == ALIGN
    assert call(short=1)[0] == WORKSPACE
    rc, outs = call(B=0)
    assert rc == OK
    for o in outs:
        assert bool((o == 7).all())
