"""
Model loading surface of the reference, kept name for name for the inference path
(/root/reference/keras_retinanet_3D/models/__init__.py:9-88):

    backbone(name)                       -> Backbone object (validate(), retinanet())
    load_model(filepath, backbone_name)  -> object with predict_on_batch([images, P_inv, planes])

`filepath` may be
    'synthetic:<seed>'   seeded random weights of the exact architecture (no trained weights ship
                         with the reference, README.md:75); 'synthetic:<seed>:trained' = the same draw with the activation statistics
                         of a trained checkpoint (per-channel scales three decades apart, dead channels, a residual stream that
                         grows stage by stage: models/weights.trained_like)
    '<file>.npz'         weights saved by models.weights.save_weights (Keras layer names)
    '<file>.h5'          a Keras model (`model.save`) or weight (`model.save_weights`) file, the format the reference reads and
                         writes (bin/convert_model.py:50-53): h5py when importable, else libhdf5 through ctypes (models/hdf5.py)
"""


class Backbone(object):
    """ This class stores additional information on backbones (reference models/__init__.py:9-39). """

    def __init__(self, backbone):
        self.backbone = backbone
        self.custom_objects = {}      # Keras deserialisation table of the reference; nothing to register here
        self.validate()

    def retinanet(self, *args, **kwargs):
        raise NotImplementedError('retinanet method not implemented.')

    def download_imagenet(self):
        raise NotImplementedError('download_imagenet method not implemented.')

    def validate(self):
        raise NotImplementedError('validate method not implemented.')


def backbone(backbone_name):
    """ Returns a backbone object for the given backbone (reference models/__init__.py:42-56). """
    if 'resnet' in backbone_name:
        from .resnet import ResNetBackbone as b
    elif 'densenet' in backbone_name:
        from .densenet import DenseNetBackbone as b
    elif 'mobilenet' in backbone_name and '_' in backbone_name:
        from .mobilenet import MobileNetBackbone as b
    elif 'mobilenet' in backbone_name:
        # (the reference cannot build such a name either: float(backbone.split('_')[1]), its models/mobilenet.py:94)
        raise NotImplementedError('Backbone class for  \'{}\' not implemented: a MobileNet name carries its width multiplier, '
                                  '\'mobilenet224_1.0\' (the multiplier is missing).'.format(backbone_name))
    else:
        raise NotImplementedError('Backbone class for  \'{}\' not implemented.'.format(backbone_name))
    return b(backbone_name)


def load_model(filepath, backbone_name='resnet50', convert=False, nms=True, class_specific_filter=True,
               orientation_specific_filter=False, dtype=None, on_range_event=None, plan=None, pose=False, range_audit=False, cuboid_nms=None,
               track=None):
    """ Loads a RetinaNet-3D inference model (reference models/__init__.py:59-88).

    `convert` is accepted for signature compatibility: every model this function returns already
    contains the decode / NMS / ground-plane-polling stages (`retinanet_bbox`, retinanet.py:359-422).
    `backbone_name`: 'resnet50' | 'resnet101' | 'resnet152' | 'densenet121' | 'densenet169' | 'densenet201' |
    'mobilenet{128,160,192,224}_{0.25,0.5,0.75,1.0}' (DenseNet and MobileNet: dtype 'f32', 'f16x3' or 'bf16x3' only).
    `dtype` (not in the reference; None = the environment's GPP_DTYPE, else 'f16x3'):
        'f16x3' (default)  float32-sized storage, every float32 product as three IEEE-half matrix products: the fastest type whose
                           detections, plane indices and 3-D corners stay within BASELINE's tolerance of the float32 path
        'f32'              float32 storage and operands (the reference's floatx, /root/reference/keras_retinanet_3D/utils/image.py:47)
        'bf16x3'           three bf16 products per float32 product (~2^-16): same detections and planes, corners off by millimetres
        'f16' | 'bf16'     16-bit storage and MFMA operands, float32 accumulation: 2.4x faster, a few percent of the detections differ
    `on_range_event` (not in the reference; dtype='f16x3' only; None = the environment's GPP_ON_RANGE_EVENT, else 'f32'): what a call does
    when one of its activations left the IEEE-half range (beyond +-65504: clamped, counted by the kernels' epilogues) --
        'f32' (default)    the call is run again on a float32 twin of the model and THAT result is returned (the reference's answer, slower)
        'raise'            GppError;      'ignore'   the clamped result is returned (model.x3_range_events() still counts)
    `range_audit` (not in the reference; dtype='f16x3' only, default False): the LOWER range of the type, opt-in.  Below 2^-14 the (hi, lo)
    half pair is a fixed-point number with a quantum of 2^-24; such a model's plans also measure the largest |x| of every channel of every
    map an x3 convolution reads (gpp_channel_absmax: one extra pass over each map, the fused bottlenecks as their separate launches; the
    results are byte for byte those of the ordinary plans) and model.range_audit() returns the report.  A synchronous call
    (predict_on_batch / _on_frames, predict_poses_*) whose run left the largest value of a whole MAP below 2^-9 -- the map is stored at
    bf16x3 grade or worse -- does what `on_range_event` says ('f32': the float32 twin's result, 'raise': GppError naming the maps,
    'ignore': the result, the report kept); model.small_magnitude_events counts such (call, map) pairs.  A sufficient condition for
    damage, not a necessary one: a few tiny channels with huge weights inside a map of ordinary size are reported (`small_channels`) and
    do not trigger.  FramePipeline and ShardedModel refuse an audit model.
    `plan` (not in the reference; None = the environment's GPP_PLAN, else 'throughput'): how the layers are launched --
        'throughput'       (default) the plan every batched caller wants: split-K only where a layer's grid is tiny at ANY batch
        'latency'          for callers that time ONE image per call, as the reference does (bin/run_network.py:108-111): the deep-K layers whose
                           batch-1 grid leaves most of the 256 CUs idle (res4 / res5 bottlenecks, P4 ... P7, the lateral 1x1s) split their K
                           loop over more workgroups.  The split is a rule of (layer, plan) -- never of the batch, the tile or a timing -- so a
                           model gives byte-identical results at every batch size and on every rank WITHIN its plan mode; between the two modes
                           results differ by float32 summation order only (both inside the parity bars, tests/test_latency_plan_gpu.py)
    `pose` (not in the reference; default False): the plan ends with the pose stage (gpp_pose_f32: what bin/run_network.py does on the host
    after predict_on_batch, on the device) and the model has predict_poses_on_batch / predict_poses_on_frames, which return one
    (B, 100, 36) table of rows (include/gpp.h) and the number of detections per image.  predict_on_batch is unchanged either way.
    `cuboid_nms` (not in the reference; default None; needs pose=True): a pair (metric, threshold), metric 'bev' or '3d' -- the plan ends
    with one more op, a greedy NMS of the cuboids themselves on the pose rows (gpp_cuboid_nms_f64): in score order
    a row is dropped when a kept row overlaps it by more than the threshold in the bird's-eye view ('bev') or in 3-D ('3d').  Every reader of
    the rows (predict_poses_*, score_poses_on_frames, predict_composites_on_frames) sees the suppressed set; model.cuboid_suppressors()
    says which row removed which.  There is no default threshold: it depends on the checkpoint.  predict_on_batch is unchanged.
    `track` (not in the reference; default None; needs pose=True): a pair (metric, threshold) or a dict {'metric': 'bev' | '3d' | 'dist',
    'threshold': T, 'max_age': 2, 'gains': (a, b, c), 'birth_score': 0.0, 'smooth': False, 'assign': 'greedy'} -- the model gets predict_tracks_on_frames /
    predict_tracks_on_batch, which follow the plan with one more launch (gpp_track_f64): the rows of every image
    are associated greedily with the cuboids carried over from the frames before (overlap above T for 'bev' / '3d', centre distance on the
    ground below T metres for 'dist') and get an identity that persists; a fixed-gain filter carries each cuboid.  The images of a call
    are consecutive frames of the model's one sequence and a later call continues it; model.reset_tracks() starts a new one,
    model.track_state() reads the state.  There is no default threshold: it depends on the checkpoint and the frame rate; the default
    gains and max_age come from synthetic scenes only.  'assign': 'optimal' launches gpp_track_optimal_f64 instead (section 4.32): the
    optimal one-to-one assignment of every frame in the place of the greedy pass, all else the same step.  'ego': True (section 4.33): the two
    methods take ego=records, (B, 16) float64 -- utils.track.ego_records of the camera-from-previous-camera transforms, or
    utils.oxts.camera_ego from KITTI's oxts and calib files -- and launch gpp_track_ego_f64: the carried cuboids are moved into every
    frame's camera coordinates before they are matched, so a parked car keeps its id from a driving camera; a missing ego on such a model
    and a given one on any other are refused.  'filter': 'kalman' with 'noise': {'radial': (r0, r1), 'tangential': (t0, t1), 'process':
    (q_pos, q_vel), 'birth_speed': v0} (section 4.34; no defaults: nothing here has seen a real sequence) launches gpp_track_kf_f64: every
    carried cuboid keeps the covariance of (x, z, vx, vz), a row's noise grows with its range along the viewing ray, and the fourth
    metric 'maha' gates at T standard deviations; model.track_covariance() reads the covariances.  Every other method is unchanged and does not touch the tracker.  FramePipeline and
    ShardedModel refuse such a model: they reorder or split the frames.
    """
    import os
    if dtype is None:
        dtype = os.environ.get('GPP_DTYPE', 'f16x3')
    from . import weights as W
    from .retinanet import RetinaNet3D
    b = backbone(backbone_name)
    name = b.backbone if W.is_mobilenet(b.backbone) else b.backbone.split('_')[0]      # (a MobileNet name carries its width multiplier)
    if isinstance(filepath, dict):
        w = filepath
    elif isinstance(filepath, str) and filepath.startswith('synthetic'):
        seed, family = W.parse_synthetic(filepath)         # 'synthetic:7', 'synthetic:7:trained', also 'synthetic:7.h5' (run_network strips 3 chars)
        w = W.synthetic_weights(name, seed, family)
    else:
        w = W.load_weights(filepath)
    model = RetinaNet3D(w, backbone_name=name, dtype=dtype, nms=nms, class_specific_filter=class_specific_filter,
                        orientation_specific_filter=orientation_specific_filter, on_range_event=on_range_event, plan=plan, pose=pose, range_audit=range_audit,
                        cuboid_nms=cuboid_nms, track=track)
    if convert:
        model.summary()
    return model
