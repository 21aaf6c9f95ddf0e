"""
Oracle of the DenseNet backbones (a helper of the DenseNet tests, not a test module): a literal PyTorch-CPU restatement of
keras.applications.densenet.DenseNet as the reference instantiates it (/root/reference/keras_retinanet_3D/models/densenet.py:62-94):
    ZeroPadding2D(3), conv1/conv 7x7/2 valid, conv1/bn, ReLU, ZeroPadding2D(1), pool1 MaxPool 3x3/2 valid;
    dense layer convS_blockI: _0_bn, ReLU, _1_conv 1x1, _1_bn, ReLU, _2_conv 3x3 'same', concatenation [x, new];
    transition poolS: _bn, ReLU, _conv 1x1, AveragePooling2D(2, 2) valid;
every BatchNormalization frozen and applied literally with epsilon 1.001e-5, no convolution bias.  C3, C4, C5 are the raw concatenations
at the end of blocks conv3, conv4, conv5.  The FPN and the heads are oracle.net_torch.Net's, unchanged (they key on layer names).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import decode_np
from oracle.net_torch import Net, _conv
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import anchors as A

EPS = 1.001e-5


class DenseNetNet(Net):
    def __init__(self, weights, backbone='densenet121', precision='f32'):
        super(DenseNetNet, self).__init__(weights, backbone, None, precision)

    def bn(self, x, name):
        g, b, m, v = (torch.as_tensor(self.w[name + '/' + p]) for p in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
        return (x - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + EPS) * g[None, :, None, None] + b[None, :, None, None]

    def resnet(self, x):
        """ the backbone hook of Net.forward: (C2, C3, C4, C5) = the four block concatenations """
        w = self.w
        x = torch.relu(self.bn(_conv(x, w['conv1/conv/kernel'], stride=2, pad=3), 'conv1/bn'))
        x = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)
        outs = []
        for stage, n in enumerate(W.DENSENET_BLOCKS[self.backbone]):
            for i in range(1, n + 1):
                nm = 'conv{}_block{}'.format(stage + 2, i)
                y = _conv(torch.relu(self.bn(x, nm + '_0_bn')), w[nm + '_1_conv/kernel'])
                y = _conv(torch.relu(self.bn(y, nm + '_1_bn')), w[nm + '_2_conv/kernel'], pad=1)
                x = torch.cat([x, y], dim=1)
            outs.append(x)
            if stage < 3:
                nm = 'pool{}'.format(stage + 2)
                x = F.avg_pool2d(_conv(torch.relu(self.bn(x, nm + '_bn')), w[nm + '_conv/kernel']), 2, 2)
        return outs


def forward(weights, images_nhwc, backbone='densenet121', precision='f32'):
    """ head tensors (+ C2..C5 and P3..P7, NHWC) of the whole graph, as oracle.net_torch.forward returns them """
    return DenseNetNet(weights, backbone, precision).forward(images_nhwc, keep_features=True)


def anchors_of(out):
    """ the anchors of the oracle's own feature maps (the reference's Anchors layers read the shapes of P3..P7) """
    return A.anchors_for_shapes([tuple(out[k].shape[1:3]) for k in ('P3', 'P4', 'P5', 'P6', 'P7')])


def detect(out):
    return decode_np.detect(out['classification_logits'], out['regression'], out['regression_dim'], anchors_of(out))
