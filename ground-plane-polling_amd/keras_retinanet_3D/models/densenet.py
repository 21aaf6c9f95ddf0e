"""
DenseNet backbones (reference models/densenet.py:24-94).  The reference builds keras.applications.densenet.DenseNet and takes the raw
concatenations at the end of dense blocks 3, 4 and 5 as C3, C4, C5; here the backbone is part of the device plan built by
models/builder.py (PlanBuilder.densenet_backbone) from the layer inventory in models/weights.py.
"""

from . import Backbone
from .weights import DENSENET_BLOCKS

allowed_backbones = {name: list(blocks) for name, blocks in DENSENET_BLOCKS.items()}


class DenseNetBackbone(Backbone):
    """ Describes backbone information and provides utility functions. """

    def retinanet(self, *args, **kwargs):
        """ Returns a retinanet model using the correct backbone. """
        return densenet_retinanet(*args, backbone=self.backbone, **kwargs)

    def validate(self):
        """ Checks whether the backbone string is correct (reference models/densenet.py:50-57). """
        backbone = self.backbone.split('_')[0]
        if backbone not in allowed_backbones:
            raise ValueError('Backbone (\'{}\') not in allowed backbones ({}).'.format(backbone, sorted(allowed_backbones)))


def densenet_retinanet(num_classes=1, backbone='densenet121', weights='synthetic:1234', **kwargs):
    """ Constructs a RetinaNet-3D inference model using a densenet backbone. """
    if num_classes != 1:
        raise NotImplementedError('one object class (the reference\'s only trained configuration)')
    from . import load_model
    return load_model(weights, backbone_name=backbone, **kwargs)
