"""
DenseNet-121/169/201 backbones (reference models/densenet.py), the parts that need no GPU: the Keras layer inventory and its parameter
counts, the feature / anchor shapes, the synthetic draw, the ResNet draw left as it was, .h5 files whose layer names hold '/', and the
backbones that still do not exist here.
"""
import hashlib

import numpy as np
import pytest

import densenet_oracle as DO
from keras_retinanet_3D import models
from keras_retinanet_3D.models import weights as W
from keras_retinanet_3D.utils import anchors as A

MEAN = np.array([103.939, 116.779, 123.68], np.float32)


@pytest.mark.parametrize('backbone,params,widths', [('densenet121', 7033408, (512, 1024, 1024)),
                                                    ('densenet169', 12636224, (512, 1280, 1664)),
                                                    ('densenet201', 18314304, (512, 1792, 1920))])
def test_inventory_matches_keras(backbone, params, widths):
    """ Keras' published include_top=False counts minus the final 'bn' (4 x C5): the backbone up to conv5_block{N}_concat """
    assert W.backbone_parameter_count(backbone) == params
    assert tuple(W.densenet_widths(backbone)[1:]) == widths
    layers = W.densenet_layers(backbone)
    blocks = W.DENSENET_BLOCKS[backbone]
    assert sum(1 for kind, _, _ in layers if kind == 'conv') == 1 + 2 * sum(blocks) + 3
    assert layers[0][1] == 'conv1/conv' and layers[-1][1] == 'conv5_block{}_2_conv'.format(blocks[3])
    fpn = {name: cin for name, _, cin, _, _ in W.fpn_layers(backbone)}
    assert (fpn['C3_reduced'], fpn['C4_reduced'], fpn['C5_reduced'], fpn['P6']) == widths + (widths[2],)
    assert W.fpn_layers() == W.fpn_layers('resnet50')          # the ResNet table, unchanged
    W.validate_weights(W.synthetic_weights(backbone, 3), backbone)


def test_shapes_and_anchors_at_402x1333():
    c = A.densenet_feature_shapes((402, 1333))
    assert c == [(50, 167), (25, 83), (12, 41)]
    shapes = A.pyramid_shapes_of_features(c)
    assert shapes == [(50, 167), (25, 83), (12, 41), (6, 21), (3, 11)]
    assert len(A.anchors_for_shapes(shapes)) == 132912
    # the ResNet pyramid of the same frame, through the same helper: unchanged
    r = A.pyramid_shapes((402, 1333))
    assert A.pyramid_shapes_of_features(r[:3]) == r and np.array_equal(A.anchors_for_shapes(r), A.anchors_for_image((402, 1333)))
    assert len(A.anchors_for_image((402, 1333))) == 137256


@pytest.mark.parametrize('hw', [(64, 96), (67, 101)])
def test_oracle_shapes_match_the_helper(hw):
    """ (64, 96): conv1 32 x 48, even sides, where the symmetric pad-1 pool and TF's 'same' pool differ; (67, 101): odd sides """
    img = np.random.default_rng(1).integers(0, 256, size=(1,) + hw + (3,)).astype(np.float32) - MEAN
    out = DO.forward(W.synthetic_weights('densenet121', 5), img, 'densenet121')
    assert [tuple(out[k].shape[1:3]) for k in ('C3', 'C4', 'C5')] == A.densenet_feature_shapes(hw)
    assert [tuple(out[k].shape[1:3]) for k in ('P3', 'P4', 'P5', 'P6', 'P7')] == A.pyramid_shapes_of_features(A.densenet_feature_shapes(hw))
    assert out['classification_logits'].shape[1] == len(DO.anchors_of(out))
    assert [out[k].shape[3] for k in ('C2', 'C3', 'C4', 'C5')] == W.densenet_widths('densenet121')


def test_resnet_synthetic_draw_unchanged():
    """ the committed full-size fixtures depend on the ResNet draws: byte-identical to before DenseNet was added """
    w = W.synthetic_weights('resnet50', 1234)
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(w[k].tobytes())
    assert h.hexdigest() == 'fb596064d94d255a78cbc7b6e06b7d2247b597ddf85a22a856a47fe441c3eca3'


def test_synthetic_draw_is_seeded_and_trained_family_rescales():
    a, b = W.synthetic_weights('densenet121', 7), W.synthetic_weights('densenet121', 7)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    t = W.synthetic_weights('densenet121', 7, 'trained')
    assert set(t) == set(a)
    g = t['conv3_block1_1_bn/gamma'] / np.maximum(a['conv3_block1_1_bn/gamma'], 1e-30)
    assert g.max() / max(g[g > 0].min(), 1e-30) > 100          # three decades between channels of one map


@pytest.mark.parametrize('backbone', ['densenet121'])
def test_h5_round_trip_with_slash_names(tmp_path, backbone):
    """ Keras DenseNet layer names hold '/' ('conv1/conv'): keys come from the layer names the file gives (h5py path, else libhdf5) """
    w = W.synthetic_weights(backbone, 11)
    path = str(tmp_path / 'd.h5')
    try:
        W.save_keras_h5(path, w)
    except OSError as exc:         # no HDF5 library on this machine at all
        pytest.skip(str(exc))
    back = W.load_keras_h5(path)
    assert 'conv1/conv/kernel' in back and 'conv1/bn/moving_variance' in back
    assert set(back) == set(w)
    assert all(np.array_equal(back[k], w[k]) for k in w)
    W.validate_weights(back, backbone)


def test_weight_keys_of_resnet_files_unchanged():
    assert W._weight_key('res2a_branch2a', 'res2a_branch2a/kernel:0') == 'res2a_branch2a/kernel'
    assert W._weight_key('regression_submodel', 'pyramid_regression_0/kernel:0') == 'pyramid_regression_0/kernel'
    assert W._weight_key('bn_conv1', 'bn_conv1/moving_mean:0') == 'bn_conv1/moving_mean'
    assert W._weight_key('conv1/conv', 'conv1/conv/kernel:0') == 'conv1/conv/kernel'


def test_backbone_dispatch():
    assert models.backbone('densenet121').backbone == 'densenet121'
    with pytest.raises(ValueError):
        models.backbone('densenet64')
    for name in ('vgg16', 'mobilenet224'):
        with pytest.raises(NotImplementedError):
            models.backbone(name)


@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
def test_16_bit_storage_is_refused(dtype):
    from keras_retinanet_3D.models.retinanet import RetinaNet3D
    with pytest.raises(ValueError, match="'f32', 'f16x3' or 'bf16x3'"):
        RetinaNet3D(W.synthetic_weights('densenet121', 1), backbone_name='densenet121', dtype=dtype)


def test_synthetic_calibration():
    """ about 10^3 anchors per 402x1333 noise frame above the 0.05 score threshold (the target of the ResNet draws), float32 oracle """
    img = np.random.default_rng(0).integers(0, 256, size=(1, 402, 1333, 3)).astype(np.float32) - MEAN
    out = DO.forward(W.synthetic_weights('densenet121', 1234), img, 'densenet121')
    p = 1.0 / (1.0 + np.exp(-out['classification_logits'].reshape(1, -1, 8)))
    n = int((p.max(axis=2) > 0.05).sum())
    assert 500 <= n <= 2000, n
