"""
MobileNet backbones (reference models/mobilenet.py:27-111).  The reference builds keras.applications.mobilenet.MobileNet(alpha,
include_top=False) and takes conv_pw_5_relu, conv_pw_11_relu and conv_pw_13_relu as C3, C4, C5; here the backbone is part of the device
plan built by models/builder.py (PlanBuilder.mobilenet_backbone) from the layer inventory in models/weights.py: one fused launch per
depthwise-separable block (csrc/mobilenet.hip).

A backbone name is 'mobilenet<rows>_<alpha>', e.g. 'mobilenet224_1.0'.  <rows> (128, 160, 192 or 224) only names the ImageNet weights
Keras would download and does not change the graph.  A documented narrowing: Keras accepts any float as alpha, this library the four
multipliers ImageNet weights exist for (0.25, 0.5, 0.75, 1.0).
"""

from . import Backbone
from .weights import MOBILENET_ALPHAS, MOBILENET_ROWS

allowed_backbones = list(MOBILENET_ROWS)


class MobileNetBackbone(Backbone):
    """ Describes backbone information and provides utility functions. """

    def retinanet(self, *args, **kwargs):
        """ Returns a retinanet model using the correct backbone. """
        return mobilenet_retinanet(*args, backbone=self.backbone, **kwargs)

    def validate(self):
        """ Checks whether the backbone string is correct (reference models/mobilenet.py:70-77). """
        rows, _, alpha = self.backbone.partition('_')
        if rows not in allowed_backbones:
            raise ValueError('Backbone (\'{}\') not in allowed backbones ({}).'.format(rows, allowed_backbones))
        try:
            alpha = float(alpha)
        except ValueError:
            alpha = None
        if alpha not in MOBILENET_ALPHAS:
            raise ValueError('Backbone (\'{}\'): width multiplier must be one of {}.'.format(self.backbone, list(MOBILENET_ALPHAS)))


def mobilenet_retinanet(num_classes=1, backbone='mobilenet224_1.0', weights='synthetic:1234', **kwargs):
    """ Constructs a RetinaNet-3D inference model using a mobilenet backbone. """
    if num_classes != 1:
        raise NotImplementedError('one object class (the reference\'s only trained configuration)')
    from . import load_model
    return load_model(weights, backbone_name=backbone, **kwargs)
