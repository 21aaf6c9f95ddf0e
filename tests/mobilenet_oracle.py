"""
Oracle of the MobileNet backbones (a helper of the MobileNet tests, not a test module): a literal PyTorch-CPU restatement of
keras.applications.mobilenet.MobileNet(alpha, include_top=False) as the reference instantiates it (its models/mobilenet.py:94-111):
    conv1_pad ZeroPadding2D(1, 1), conv1 3x3 / 2 'valid' (no bias), conv1_bn, ReLU6;
    block i = 1..13: conv_pad_i ZeroPadding2D(1, 1), conv_dw_i DepthwiseConv2D 3x3 'valid' (stride 2 for i in 2, 4, 6, 12), conv_dw_i_bn,
    ReLU6, conv_pw_i 1x1, conv_pw_i_bn, ReLU6;
every BatchNormalization frozen and applied literally with epsilon 1e-3, no convolution bias.  conv_pw_3 / 5 / 11 / 13 (post-ReLU6) are
C2, C3, C4, C5.  The FPN and the heads are oracle.net_torch.Net's, unchanged.

The graph is restated FROM MEMORY of keras_applications 1.0.2 (the release Keras 2.2.0, which the reference was tested with, pins):
Keras is not installed where this project is developed, so the padding rule could not be checked against it.  Later releases pad
stride-2 layers with ((0, 1), (0, 1)) instead; the rule lives in ONE function here (`pad`) and in one in the kernels
(csrc/mobilenet.hip tap_origin) so that it can be flipped on both sides.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import decode_np
from oracle.net_torch import Net
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import anchors as A

EPS = 1e-3


def pad(x, stride):
    """ the padding in front of every 3 x 3 layer: ZeroPadding2D(1, 1), symmetric, whatever the stride """
    return F.pad(x, (1, 1, 1, 1))


def relu6(x):
    return torch.clamp(x, 0, 6)


class MobileNetNet(Net):
    def __init__(self, weights, backbone='mobilenet224_1.0', precision='f32'):
        super(MobileNetNet, self).__init__(weights, backbone, None, precision)
        self.saturation = None            # when a dict: layer name -> (share of activations == 6, share in (0, 6))

    def bn(self, x, name):
        g, b, m, v = (torch.as_tensor(self.w[name + '/' + p]) for p in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
        return (x - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS) * g[None, :, None, None] + b[None, :, None, None]

    def act(self, x, name):
        y = relu6(self.bn(x, name + '_bn'))
        if self.saturation is not None:
            self.saturation[name] = (float((y == 6).double().mean()), float(((y > 0) & (y < 6)).double().mean()))
        return y

    def depthwise_block(self, x, i, stride):
        dw = torch.as_tensor(self.w['conv_dw_{}/depthwise_kernel'.format(i)])                 # (3, 3, C, 1)
        x = F.conv2d(pad(x, stride), dw.permute(2, 3, 0, 1).contiguous(), None, stride=stride, groups=x.shape[1])
        x = self.act(x, 'conv_dw_{}'.format(i))
        pw = torch.as_tensor(self.w['conv_pw_{}/kernel'.format(i)])                           # (1, 1, C_in, C_out)
        return self.act(F.conv2d(x, pw.permute(3, 2, 0, 1).contiguous()), 'conv_pw_{}'.format(i))

    def resnet(self, x):
        """ the backbone hook of Net.forward: (C2, C3, C4, C5) = conv_pw_3 / 5 / 11 / 13 behind their ReLU6 """
        k = torch.as_tensor(self.w['conv1/kernel'])
        x = self.act(F.conv2d(pad(x, 2), k.permute(3, 2, 0, 1).contiguous(), None, stride=2), 'conv1')
        outs = []
        for i, _, _, stride in W.mobilenet_blocks(self.backbone):
            x = self.depthwise_block(x, i, stride)
            if i in W.MOBILENET_TAPS:
                outs.append(x)
        return outs


def forward(weights, images_nhwc, backbone='mobilenet224_1.0', precision='f32', saturation=None):
    """ head tensors (+ C2..C5 and P3..P7, NHWC) of the whole graph, as oracle.net_torch.forward returns them """
    net = MobileNetNet(weights, backbone, precision)
    net.saturation = saturation
    return net.forward(images_nhwc, keep_features=True)


def anchors_of(out):
    return A.anchors_for_shapes([tuple(out[k].shape[1:3]) for k in ('P3', 'P4', 'P5', 'P6', 'P7')])


def detect(out):
    return decode_np.detect(out['classification_logits'], out['regression'], out['regression_dim'], anchors_of(out))
