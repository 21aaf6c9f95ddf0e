""" What the tile tuner and the head-form rule do without a GPU: the tune cache's file format and its load / save logic
(models/tuning.TuneCache: what profiles/*/tile_choices_*.json and every GPP_TUNE_CACHE file are written in), the configuration part of
its keys (PlanOptions.tune_key) as literals, and plan.head_forms against the plans the builder makes and against each of its refusing
conditions. """
import glob
import json
import os

import pytest
import torch

import helpers
from keras_retinanet_3D import models
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import plan as P
from keras_retinanet_3D.models import tuning
from keras_retinanet_3D.models import weights as W


@pytest.fixture(scope='module')
def cpu_model():
    """ model_for(dtype, kwargs, env, backbone): a CPU model built under `env` (the cache's configuration is read when a model is made) """
    weights = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, 'require_device', lambda: torch.device('cpu'))
        for k in [k for k in os.environ if k.startswith('GPP_') and k != 'GPP_LIB']:
            mp.delenv(k)
        mp.setenv('GPP_AUTOTUNE', '0')

        def model_for(dt='f16x3', kw=None, env=None, bb='resnet50'):
            if bb not in weights:
                weights[bb] = W.synthetic_weights(bb, 1234)
            with pytest.MonkeyPatch.context() as inner:
                for k, v in (env or {}).items():
                    inner.setenv(k, v)
                return models.load_model(weights[bb], backbone_name=bb, dtype=dt, **(kw or {}))
        yield model_for


# ---------------------------------------------------------------------------------------------------- the cache and its file
CFG = 'v2;0123456789ab;x3split=2;fuse=64,128/64,128;plan=throughput'
ENTRIES = {('P3', 8, 402, 1333): (1192256, 271.44), ('res4a_branch2a', 4, 402, 1333): (64128, 23.08), ('pyramid_regression_3@rows', 4, 224, 352): (5, 40.5)}


def saved(path, config=CFG, backbone='resnet50', dtype='f16x3', entries=ENTRIES):
    cache = tuning.TuneCache(config, backbone, dtype)
    for key, val in entries.items():
        cache.put(key, val)
    cache.save(path)
    return cache


def loaded(path, config=CFG, backbone='resnet50', dtype='f16x3'):
    cache = tuning.TuneCache(config, backbone, dtype)
    cache.load(path)
    return cache.entries


def test_entries_come_back_under_the_same_configuration_backbone_and_type_only(tmp_path):
    path = str(tmp_path / 'tiles.json')
    assert loaded(path) == {}                                   # no file yet
    saved(path)
    assert loaded(path) == ENTRIES
    assert all(type(t) is int and type(us) is float for t, us in loaded(path).values())
    assert loaded(path, config=CFG.replace('x3split=2', 'x3split=1')) == {}
    assert loaded(path, config=CFG.replace('0123456789ab', 'ba9876543210')) == {}
    assert loaded(path, backbone='resnet101') == {}
    assert loaded(path, dtype='bf16x3') == {}
    with open(path) as f:
        data = json.load(f)
    assert data == {'|'.join([CFG, 'resnet50', 'f16x3', name, str(b), str(h), str(w)]): [tile, us] for (name, b, h, w), (tile, us) in ENTRIES.items()}
    assert glob.glob(str(tmp_path / '*.tmp.*')) == []
    tuning.TuneCache(CFG, 'resnet50', 'f16x3').load(None)       # GPP_TUNE_CACHE unset: nothing to read, nothing to write
    tuning.TuneCache(CFG, 'resnet50', 'f16x3').save(None)


def test_save_keeps_what_the_file_held_and_load_takes_the_current_keys_only(tmp_path):
    path = str(tmp_path / 'tiles.json')
    foreign = 'v2;ffffffffffff;x3split=2;fuse=64,128/64,128;plan=throughput|resnet50|f16x3|P3|8|402|1333'
    old = 'resnet50|bf16|C3_reduced|8|402|1333'                 # profiles/r1/tile_choices_b8_resnet50.json: six fields, [tile, split_k, us]
    current = CFG + '|resnet50|f16x3|P4|8|402|1333'
    with open(path, 'w') as f:
        json.dump({foreign: [64128, 1.5], old: [64128, 1, 62.71], current: [160128, 1, 77.52]}, f)
    assert loaded(path) == {('P4', 8, 402, 1333): (160128, 77.52)}          # (tile, us): the first and the LAST value of the list
    cache = tuning.TuneCache(CFG, 'resnet50', 'f16x3')
    cache.load(path)
    cache.put(('P5', 8, 402, 1333), (1128256, 41.0))
    cache.save(path)
    with open(path) as f:
        data = json.load(f)
    assert data == {foreign: [64128, 1.5], old: [64128, 1, 62.71], current: [160128, 77.52], CFG + '|resnet50|f16x3|P5|8|402|1333': [1128256, 41.0]}
    assert loaded(path) == {('P4', 8, 402, 1333): (160128, 77.52), ('P5', 8, 402, 1333): (1128256, 41.0)}
    assert glob.glob(str(tmp_path / '*.tmp.*')) == []


def test_a_file_that_is_not_json_does_not_stop_save(tmp_path):
    path = str(tmp_path / 'tiles.json')
    with open(path, 'w') as f:
        f.write('{"torn')
    saved(path)
    assert loaded(path) == ENTRIES
    assert glob.glob(str(tmp_path / '*.tmp.*')) == []


def test_only_rank_0_writes(tmp_path, monkeypatch):
    path = str(tmp_path / 'tiles.json')
    monkeypatch.setenv('RANK', '1')
    saved(path)
    assert os.listdir(str(tmp_path)) == []
    monkeypatch.setenv('RANK', '0')
    saved(path)
    assert os.listdir(str(tmp_path)) == ['tiles.json']


def test_a_model_reads_its_cache_file_once_when_it_is_made(tmp_path, cpu_model):
    path = str(tmp_path / 'tiles.json')
    config = cpu_model()._tune.config
    assert config == 'v2;{};x3split=2;fuse=64,128/64,128;plan=throughput'.format(hip.lib().gpp_version().decode().split('src:')[-1])
    saved(path, config=config)
    assert cpu_model(env={'GPP_TUNE_CACHE': path})._tune.entries == ENTRIES
    assert cpu_model(env={'GPP_TUNE_CACHE': path, 'GPP_X3_SPLIT': '1'})._tune.entries == {}
    assert cpu_model(dt='bf16x3', env={'GPP_TUNE_CACHE': path})._tune.entries == {}
    assert cpu_model()._tune.entries == {}


# ---------------------------------------------------------------------------------------------------- the configuration in the keys
DEFAULT_KEY = 'x3split=2;fuse=64,128/64,128;plan=throughput'


@pytest.mark.parametrize('kw, env, key', [
    ({}, {}, DEFAULT_KEY),
    ({}, {'GPP_X3_SPLIT': '1'}, 'x3split=1;fuse=64,128/64,128;plan=throughput'),
    ({}, {'GPP_FUSE_TAIL': ''}, 'x3split=2;fuse=/64,128;plan=throughput'),
    ({}, {'GPP_FUSE_BLOCK': ''}, 'x3split=2;fuse=64,128/;plan=throughput'),
    ({}, {'GPP_FUSE_BLOCK_INPROJ': '0'}, DEFAULT_KEY + ';inproj=0'),
    ({'range_audit': True}, {}, DEFAULT_KEY + ';audit'),
    ({'plan': 'latency'}, {}, 'x3split=2;fuse=64,128/64,128;plan=latency;lat=2048,512,8,512'),
    ({'plan': 'latency'}, {'GPP_LAT_TARGET': '256'}, 'x3split=2;fuse=64,128/64,128;plan=latency;lat=2048,256,8,512'),
], ids=lambda v: ' '.join('{}={}'.format(*kv) for kv in sorted(v.items())) or 'default' if isinstance(v, dict) else None)
def test_tune_key_literals(kw, env, key, cpu_model, monkeypatch):
    """ the strings the code before models/tuning.py gave: every cache file written since carries them in its keys """
    model = cpu_model(kw=kw)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert model._plan_options(1).tune_key == model._plan_options(8).tune_key == key
    assert cpu_model(dt='bf16', kw={k: v for k, v in kw.items() if k != 'range_audit'})._plan_options(2).tune_key == key.replace(';audit', '')


# ---------------------------------------------------------------------------------------------------- head_forms
Z = {'GPP_SPARSE_TOWER_MIN_ROUNDS': '0', 'GPP_SPARSE_TOWER_DEEP_MIN_ROUNDS': '0'}
HEAD_LAYERS = P.HEAD_OUTPUTS + ('pyramid_regression_1', 'pyramid_regression_2', 'pyramid_regression_3')
# (backbone, dtype, model keywords, environment, B, H, W) -> (gathered output layers, tower layers of both forms, deep layers,
# pyramid_classification makes the deep lists), None: no sparse head outputs at all -- what the plans of the builder before head_forms carried
FORMS = [
    (('resnet50', 'f16x3', {}, Z, 1, 224, 352), (2, 1, 0, False)),
    (('resnet50', 'f16x3', {}, Z, 4, 224, 352), (2, 1, 2, True)),
    (('resnet50', 'bf16x3', {}, Z, 4, 224, 352), (2, 1, 2, True)),
    (('resnet50', 'bf16', {}, Z, 4, 224, 352), (2, 0, 0, False)),
    (('resnet50', 'f32', {}, Z, 4, 224, 352), (2, 0, 0, False)),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_SPARSE_TOWER_DEPTH='1'), 4, 224, 352), (2, 1, 0, False)),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_SPARSE_TOWER_DEPTH='2'), 4, 224, 352), (2, 1, 1, True)),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_SPARSE_TOWER='0'), 4, 224, 352), (2, 0, 0, False)),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_SPARSE_HEADS='0'), 4, 224, 352), None),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_CLS_LANE='1'), 4, 224, 352), (2, 1, 0, False)),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_HEAD_LANES='1'), 4, 224, 352), None),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_X3_SPLIT='0'), 4, 224, 352), (2, 0, 0, False)),
    (('resnet50', 'f16x3', {}, dict(Z, GPP_DECODE_OVERLAP='0'), 4, 224, 352), None),
    (('resnet50', 'f16x3', {'plan': 'latency'}, Z, 4, 224, 352), (1, 0, 0, False)),
    (('resnet50', 'f16x3', {'orientation_specific_filter': True}, Z, 4, 224, 352), None),
    (('densenet121', 'f16x3', {}, Z, 2, 224, 352), (2, 1, 0, False)),
    (('mobilenet224_1.0', 'f16x3', {}, Z, 4, 224, 352), (2, 1, 2, True)),
    (('resnet50', 'f16x3', {}, {}, 4, 224, 352), (2, 0, 0, False)),
    (('resnet50', 'f16x3', {'pose': True}, {}, 2, 200, 333), (1, 0, 0, False)),
    (('resnet50', 'f16x3', {'range_audit': True}, {}, 2, 200, 333), None),
]


def test_the_form_rows_are_rows_of_the_plan_matrix():
    labels = {helpers.plan_label(cfg) for cfg in helpers.plan_matrix()}
    assert all(helpers.plan_label(cfg) in labels for cfg, _ in FORMS)


@pytest.mark.parametrize('cfg, want', FORMS, ids=[helpers.plan_label(cfg) for cfg, _ in FORMS])
def test_head_forms_names_what_the_plan_carries(cfg, want, cpu_model, monkeypatch):
    bb, dt, kw, env, B, H, Wd = cfg
    model = cpu_model(dt, kw, bb=bb)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = model.plan_for(B, H, Wd, 100, True)
    model._plans.clear()
    levels = [(plan.features[p].H, plan.features[p].W) for p in ('P3', 'P4', 'P5', 'P6', 'P7')]
    forms = P.head_forms(model._plan_options(B), model.dtype, model.plan_mode, model.osf, model.audit,
                         {n: model.conv_w[n][2] for n in HEAD_LAYERS}, hasattr(hip.lib(), 'gpp_detect_deep_lists'), levels, B)
    sp = plan.sparse
    lists_after = [bool(d.lists_after) for kind, _, d, name, _ in plan.ops if name == 'pyramid_classification']
    assert len(lists_after) == 1
    carried = None if sp is None else (len(sp.gathered), len(sp.tower), sp.deep_layers, lists_after[0])
    assert carried == want
    assert forms.sparse == (sp is not None)
    assert sorted(forms.outputs) == sorted(P.HEAD_OUTPUTS) and forms.outputs['pyramid_classification'] in ('dense', 'lists_after')
    named = (sum(f == 'pair' for f in forms.outputs.values()), int(forms.tower_both), forms.deep_layers,
             forms.outputs['pyramid_classification'] == 'lists_after')
    assert named == (want or (0, 0, 0, False))
    if sp is not None:
        assert [d.KH * d.KW * d.C_in for d in sp.deep] == [9 * 512] * forms.deep_layers and len(sp.dense) == len(sp.gathered)


LEVELS = [(28, 44), (14, 22), (7, 11), (4, 6), (2, 3)]          # 224 x 352
SHAPES = dict({n: (3, 3, 512, 512) for n in HEAD_LAYERS}, pyramid_classification=(3, 3, 256, 96), pyramid_regression_ops=(3, 3, 512, 144),
              pyramid_regression_dim=(3, 3, 128, 36))


def options(**fields):
    """ the switches head_forms reads, at what a default f16x3 plan of B >= 3 has them with both round thresholds at 0 """
    base = dict(sparse_heads=0.5, sparse_tower=0.75, sparse_tower_rounds=0.0, sparse_deep=0.75, sparse_deep_rounds=0.0, sparse_depth=3,
                decode_overlap=True, x3_level=2, cls_lane=0, head_lanes=False)
    return P.PlanOptions(**{f: dict(base, **fields).get(f) for f in P.PlanOptions._fields})


def forms_of(opts=None, dtype='f16x3', plan_mode='throughput', osf=False, audit=False, layers=SHAPES, deep_lists=True, levels=LEVELS, B=4):
    return P.head_forms(opts or options(), dtype, plan_mode, osf, audit, layers, deep_lists, levels, B)


def test_head_forms_refuses_on_each_condition_of_its_rules():
    pair = {'pyramid_classification': 'lists_after', 'pyramid_regression_ops': 'pair', 'pyramid_regression_dim': 'pair'}
    assert forms_of() == P.HeadForms(True, pair, True, 2)
    no_deep = P.HeadForms(True, dict(pair, pyramid_classification='dense'), True, 0)
    no_tower = P.HeadForms(True, dict(pair, pyramid_classification='dense'), False, 0)
    dense = {n: 'dense' for n in P.HEAD_OUTPUTS}
    assert forms_of(options(sparse_heads=0.0, sparse_tower=0.0)) == P.HeadForms(False, dense, False, 0)
    # the tower's last layer: its reader split (a small frame: 200 x 333's levels), the layer itself split, a width that is no multiple of
    # 256, the switch, the decode overlap, a type or a plan without pre-split maps, too few rounds
    # (the split rule splits a 3 x 3 x 512 layer of at most 24 tiles of 128 x 128: at 200 x 333's 1430 pixels 144 and 256 columns are, 384 are not)
    small = [(25, 42), (13, 21), (7, 11), (4, 6), (2, 3)]
    wide_ops = dict(SHAPES, pyramid_regression_ops=(3, 3, 512, 384))
    assert forms_of(levels=small) == P.HeadForms(True, dict(dense, pyramid_regression_dim='pair'), False, 0)
    assert forms_of(levels=small, layers=wide_ops) == forms_of()
    assert forms_of(levels=small, layers=dict(wide_ops, pyramid_regression_3=(3, 3, 512, 256))) == no_tower
    assert forms_of(layers=dict(SHAPES, pyramid_regression_3=(3, 3, 512, 384))) == no_tower
    assert forms_of(options(sparse_tower=0.0)) == no_tower
    assert forms_of(options(decode_overlap=False)) == no_tower
    assert forms_of(dtype='bf16') == forms_of(dtype='f32') == no_tower and forms_of(dtype='bf16x3') == forms_of()
    assert forms_of(options(x3_level=0)) == no_tower and forms_of(options(x3_level=1)) == forms_of()
    rows = sum((4 * h * w + 255) // 256 for h, w in LEVELS)          # 29 rows of workgroups, two columns: 58 workgroups
    assert forms_of(options(sparse_tower_rounds=58 / 256.0)) == no_tower and forms_of(options(sparse_tower_rounds=57 / 256.0)) == forms_of()
    assert rows == 29 and forms_of(options(sparse_tower_rounds=1.0)) == no_tower
    # the layers in front of it: the depth, the entry point, the lanes, the two kinds of model, a split or odd layer, too few rounds
    assert forms_of(options(sparse_depth=1)) == no_deep and forms_of(options(sparse_depth=2)).deep_layers == 1
    assert forms_of(options(sparse_depth=2)).outputs == pair and forms_of(options(sparse_depth=7)).deep_layers == 2
    assert forms_of(deep_lists=False) == no_deep
    assert forms_of(options(cls_lane=2)) == no_deep and forms_of(options(head_lanes=True)) == no_deep
    assert forms_of(osf=True) == no_deep and forms_of(audit=True) == no_deep
    assert forms_of(layers=dict(SHAPES, pyramid_classification=(3, 3, 512, 96))) == no_deep
    for name in ('pyramid_regression_1', 'pyramid_regression_2'):
        assert forms_of(levels=small, layers=dict(wide_ops, **{name: (3, 3, 512, 256)})) == no_deep, name
    for name in ('pyramid_regression_1', 'pyramid_regression_2'):
        assert forms_of(layers=dict(SHAPES, **{name: (3, 3, 512, 384)})) == no_deep, name
    assert forms_of(options(sparse_deep_rounds=58 / 256.0)) == no_deep and forms_of(options(sparse_deep_rounds=57 / 256.0)) == forms_of()
    # the latency plan asks its own rule: at this size it splits pyramid_regression_ops (the 'plan=latency' row above)
    assert forms_of(plan_mode='latency') == P.HeadForms(True, dict(dense, pyramid_regression_dim='pair'), False, 0)
