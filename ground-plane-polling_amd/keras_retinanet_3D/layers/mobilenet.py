"""
Host side of the MobileNet kernels (csrc/mobilenet.hip, C ABI gpp_mobilenet_block / gpp_mobilenet_stem): weight packing and the
descriptor of one depthwise-separable block.  Plays the role of keras' DepthwiseConv2D + BatchNormalization + ReLU6 + Conv2D 1x1 +
BatchNormalization + ReLU6 of keras.applications.mobilenet; no arithmetic happens here beyond folding and splitting the weights.
"""

import numpy as np

from ..backend import hip
from . import conv as C

K_CHUNK = 32          # input channels per 128-byte chunk of a packed weight row
ROW_MULTIPLE = 256    # packed rows are zero-filled up to a multiple of the widest tile


def pack_pointwise(kernel_hwio, dtype, device):
    """ Keras (1, 1, C_in, C_out) float32 kernel (BN folded) -> (weight, out_scale or None), weight a float32-typed device tensor
    [C_out rounded up to 256][C_in rounded up to 32]: row n = output channel n in natural order, zero rows and zero channels as filling.
    'f32': the values.  'f16x3' / 'bf16x3': every 32 channels become [32 hi | 32 lo] halves, hi = h(w), lo = h(w - hi); 'f16x3' scales a
    row by the power of two layers/conv.weight_scale chooses first, and out_scale (layers/conv.out_scale_of) undoes it. """
    import torch
    k = np.ascontiguousarray(kernel_hwio, dtype=np.float32)
    assert k.shape[:2] == (1, 1)
    cin, cout = k.shape[2:]
    rows, kp = -(-cout // ROW_MULTIPLE) * ROW_MULTIPLE, -(-cin // K_CHUNK) * K_CHUNK
    w = torch.zeros((rows, kp), dtype=torch.float32)
    w[:cout, :cin] = torch.as_tensor(k[0, 0].T.copy())
    if dtype == 'f32':
        return w.to(device).contiguous(), None
    assert dtype in C.X3_TYPES
    scale = None
    if dtype == 'f16x3':
        w = w * C.weight_scale(k, rows)[:, None]                  # exact: powers of two
        scale = C.out_scale_of(k, device)
    half = C.x3_half(dtype)
    hi = w.to(half)
    lo = (w - hi.to(torch.float32)).to(half)
    both = torch.stack([hi.reshape(rows, -1, K_CHUNK), lo.reshape(rows, -1, K_CHUNK)], dim=2).reshape(rows, 2 * kp)
    return both.contiguous().view(torch.float32).to(device).contiguous(), scale


def pack_depthwise(kernel_hwc1):
    """ Keras (3, 3, C, 1) depthwise kernel (BN folded) -> [9][C] float32, tap dy * 3 + dx major """
    k = np.asarray(kernel_hwc1, dtype=np.float32)
    assert k.shape[:2] == (3, 3) and k.shape[3] == 1
    return np.ascontiguousarray(k[..., 0].reshape(9, k.shape[2]))


def out_size(n, stride):
    """ ZeroPadding2D(1) + 3 x 3 'valid' at this stride """
    return (n - 1) // stride + 1


def block_desc(inp, out, dw_w, dw_b, pw_w, pw_b, out_scale, stride, dtype, tile_hint=0):
    """ gpp_mobilenet_block_desc over two FMaps (dense over the batch) and the packed weights """
    assert inp.bstride == inp.H * inp.W * inp.pitch and out.bstride == out.H * out.W * out.pitch and not inp.split and not out.split
    assert (out.H, out.W) == (out_size(inp.H, stride), out_size(inp.W, stride)) and out.B == inp.B
    d = hip.MobileNetBlockDesc()
    esz = inp.buf.element_size()
    d.inp, d.out = inp.buf.data_ptr() + inp.off * esz, out.buf.data_ptr() + out.off * esz
    d.dw_weight, d.dw_bias, d.pw_weight, d.pw_bias = dw_w.data_ptr(), dw_b.data_ptr(), pw_w.data_ptr(), pw_b.data_ptr()
    d.out_scale = out_scale.data_ptr() if out_scale is not None else None
    d.dtype = C.gpp_dtype(dtype)
    d.B, d.H, d.W, d.C_in, d.C_out, d.stride = inp.B, inp.H, inp.W, inp.C, out.C, stride
    d.in_pitch, d.out_pitch, d.weight_rows, d.tile_hint = inp.pitch, out.pitch, int(pw_w.shape[0]), int(tile_hint)
    return d


def block_flops(d):
    ho, wo = out_size(d.H, d.stride), out_size(d.W, d.stride)
    return 2.0 * d.B * ho * wo * d.C_in * (9 + d.C_out)


def block_bytes(d):
    """ compulsory HBM bytes of one launch: input + output + weights """
    ho, wo = out_size(d.H, d.stride), out_size(d.W, d.stride)
    return 4.0 * (d.B * d.H * d.W * d.C_in + d.B * ho * wo * d.C_out + d.C_in * (10 + d.C_out) + d.C_out)
