"""
The Python side of the C ABI against include/gpp.h itself, without the built library and without a device:

  layout      every ctypes.Structure of backend/hip.py and models/plan.py, and utils/track.STATE_DTYPE: sizeof, and the offset and size of
              every field, against what the host C compiler gives for the header's struct
  constants   every GPP_* name of backend/hip.py and every OP_* code of models/plan.py against the header's #define
  signatures  every argument list backend/hip.py binds against the header's prototype: count and, per parameter, class

A kernel reads its pointers out of these descriptors: a mirror that drifts from the header is a GPU fault, not a wrong number.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.models import plan
from keras_retinanet_3D.utils import track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gpp.h')

# mirror -> the header's struct.  A ctypes.Structure of the two modules that is missing here fails test_layout: no descriptor goes unchecked
C_NAME = {
    hip.ConvGroup: 'gpp_conv_group', hip.ConvDesc: 'gpp_conv_desc', hip.PixelListDesc: 'gpp_pixel_list_desc',
    hip.DeepListDesc: 'gpp_deep_list_desc', hip.MobileNetBlockDesc: 'gpp_mobilenet_block_desc',
    hip.MobileNetStemDesc: 'gpp_mobilenet_stem_desc', hip.AbsmaxDesc: 'gpp_absmax_desc', hip.AbsmaxClearDesc: 'gpp_absmax_clear_desc',
    hip.TrackState: 'gpp_track_state', hip.TrackParams: 'gpp_track_params', hip.TrackKfParams: 'gpp_track_kf_params',
    hip.MotParams: 'gpp_mot_params',
    plan.StemDesc: 'gpp_stem_desc', plan.PoolDesc: 'gpp_pool_desc', plan.RaggedStemDesc: 'gpp_ragged_stem_desc',
    plan.RaggedPoolDesc: 'gpp_ragged_pool_desc', plan.ReluDesc: 'gpp_relu_desc', plan.DetectDesc: 'gpp_detect_desc',
    plan.CandidatePixelsDesc: 'gpp_candidate_pixels_desc', plan.PollDesc: 'gpp_poll_desc', plan.PoseDesc: 'gpp_pose_desc',
    plan.CuboidNmsDesc: 'gpp_cuboid_nms_desc', plan.PreactDesc: 'gpp_preact_desc', plan.DensePoolDesc: 'gpp_dense_pool_desc',
    plan.PlanOp: 'gpp_plan_op', plan.TailDesc: 'gpp_tail_desc', plan.BlockDesc: 'gpp_block_desc', plan.BlockProjDesc: 'gpp_block_proj_desc',
}
# the known places where a mirror's field is not spelled as the header's member: (mirror or None = all, field) -> member
C_FIELD = {(None, 'inp'): 'in', (plan.BlockDesc, 'reserved'): 'form'}
C_FIELD.update({(plan.BlockProjDesc, f): 'block.' + f for f in ('conv1x1_a', 'conv3x3_b', 'conv1x1_c', 'tile', 'form')})
# the op codes of models/plan.py that are not GPP_<their own name>
C_OP = {'OP_TAIL': 'GPP_OP_BOTTLENECK_TAIL', 'OP_BLOCK': 'GPP_OP_BOTTLENECK_BLOCK'}


def mirrors():
    return [(mod, cls) for mod in (hip, plan) for cls in vars(mod).values()
            if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls.__module__ == mod.__name__]


def member(cls, field):
    return C_FIELD.get((cls, field), C_FIELD.get((None, field), field))


def header_text():
    """ include/gpp.h without its comments """
    with open(HEADER) as f:
        return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S))


def header_defines():
    """ the object-like GPP_* macros that have a value (not the include guard, not GPP_OP_LANE(l)) """
    return re.findall(r'^#define[ \t]+(GPP_\w+)[ \t]+\S', header_text(), flags=re.M)


@pytest.fixture(scope='module')
def c_facts(tmp_path_factory):
    """ what the host C compiler says of include/gpp.h, compiled and run once: {'sizeof': {struct: bytes}, 'field': {(struct, member):
    (offset, bytes)}, 'define': {name: value}} """
    cc = shutil.which('cc') or shutil.which('clang') or shutil.which('clang', path='/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin')
    if cc is None:
        pytest.skip('no host C compiler (cc, or clang of ROCm): the header cannot be asked')
    lines = ['#include <stdio.h>', '#include "gpp.h"', 'int main(void) {']
    structs = [(name, [member(cls, f) for f, _ in cls._fields_]) for cls, name in C_NAME.items()]
    structs.append(('gpp_track_state', list(track.STATE_DTYPE.names)))
    for name, members in structs:
        lines.append('printf("sizeof {0} - %zu 0\\n", sizeof({0}));'.format(name))
        for m in members:
            lines.append('printf("field {0} {1} %zu %zu\\n", offsetof({0}, {1}), sizeof((({0}*)0)->{1}));'.format(name, m))
    for name in header_defines():
        lines.append('printf("define {0} - %lld 0\\n", (long long)({0}));'.format(name))
    lines.append('return 0; }')
    tmp = tmp_path_factory.mktemp('binding')
    src, exe = str(tmp / 'layout.c'), str(tmp / 'layout')
    with open(src, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    subprocess.check_call([cc, '-std=c99', '-I', os.path.dirname(HEADER), '-o', exe, src])
    facts = {'sizeof': {}, 'field': {}, 'define': {}}
    for line in subprocess.check_output([exe], universal_newlines=True).splitlines():
        kind, name, m, a, b = line.split()
        if kind == 'field':
            facts['field'][name, m] = (int(a), int(b))
        else:
            facts[kind][name] = int(a)
    return facts


def test_layout(c_facts):
    """ all 12 mirrors of backend/hip.py, all 16 of models/plan.py and utils/track.STATE_DTYPE: size, and every field's offset and size """
    unmapped = [mod.__name__ + '.' + cls.__name__ for mod, cls in mirrors() if cls not in C_NAME]
    assert not unmapped, 'a mirror with no entry in C_NAME: {}'.format(unmapped)
    assert len([1 for mod, _ in mirrors() if mod is hip]) >= 12 and len([1 for mod, _ in mirrors() if mod is plan]) >= 16
    wrong = []
    for cls, name in C_NAME.items():
        if ctypes.sizeof(cls) != c_facts['sizeof'][name]:
            wrong.append('sizeof {}: {} here, {} in the header'.format(cls.__name__, ctypes.sizeof(cls), c_facts['sizeof'][name]))
        for f, _ in cls._fields_:
            got, want = (getattr(cls, f).offset, getattr(cls, f).size), c_facts['field'][name, member(cls, f)]
            if got != want:
                wrong.append('{}.{}: (offset, size) {} here, {} in the header'.format(cls.__name__, f, got, want))
    if track.STATE_DTYPE.itemsize != c_facts['sizeof']['gpp_track_state']:
        wrong.append('STATE_DTYPE: {} bytes, gpp_track_state {}'.format(track.STATE_DTYPE.itemsize, c_facts['sizeof']['gpp_track_state']))
    for f in track.STATE_DTYPE.names:
        dtype, offset = track.STATE_DTYPE.fields[f][:2]
        if (offset, dtype.itemsize) != c_facts['field']['gpp_track_state', f]:
            wrong.append('STATE_DTYPE.{}: {} here, {} in the header'.format(f, (offset, dtype.itemsize), c_facts['field']['gpp_track_state', f]))
    # the row-major (fields, tracks) float64 block of the header is what both mirrors must spell
    assert track.STATE_DTYPE['box'].shape == (hip.GPP_TRACK_FIELDS, hip.GPP_TRACK_MAX_TRACKS)
    assert not wrong, '\n'.join(wrong)


def test_constants(c_facts):
    """ every GPP_* of backend/hip.py and every OP_* of models/plan.py has the header's value """
    defines = c_facts['define']
    assert len(defines) == len(header_defines()) > 100
    mine = {n: v for n, v in vars(hip).items() if n.startswith('GPP_') and isinstance(v, int)}
    assert len(mine) >= 42                  # a floor: a module that lost its names must not pass by having none
    wrong = ['hip.{} = {}, header: {}'.format(n, v, defines.get(n, 'no such #define')) for n, v in sorted(mine.items()) if defines.get(n) != v]
    ops = {n: v for n, v in vars(plan).items() if n.startswith('OP_') and isinstance(v, int)}
    assert len(ops) >= 27
    for n, v in sorted(ops.items()):
        c = C_OP.get(n, 'GPP_' + n)
        if defines.get(c) != v:
            wrong.append('plan.{} = {}, header {}: {}'.format(n, v, c, defines.get(c, 'no such #define')))
    assert {defines[c] for c in ('GPP_OP_DETECT', 'GPP_OP_DETECT_CANDIDATES', 'GPP_OP_DETECT_SELECT', 'GPP_OP_DETECT_EMIT', 'GPP_OP_DETECT_OSF',
                                 'GPP_OP_DETECT_CANDIDATE_PIXELS')} == set(plan.DETECT_OPS)
    assert not wrong, '\n'.join(wrong)


C_CLASS = {'int': 'int32', 'int32_t': 'int32', 'unsigned': 'uint32', 'unsigned int': 'uint32', 'uint32_t': 'uint32', 'size_t': 'size_t',
           'float': 'float', 'double': 'double', 'int64_t': 'int64', 'long long': 'int64'}
CTYPES_CLASS = {ctypes.c_int: 'int32', ctypes.c_uint: 'uint32', ctypes.c_size_t: 'size_t', ctypes.c_float: 'float', ctypes.c_double: 'double',
                ctypes.c_int64: 'int64', ctypes.c_longlong: 'int64'}


def prototypes():
    """ {entry point: (class of the result, [class of every parameter])} of include/gpp.h; what cannot be classified raises """
    text = re.sub(r'^[ \t]*#[^\n]*(\\\n[^\n]*)*', '', header_text(), flags=re.M)
    found = {}
    for result, name, params in re.findall(r'([\w \t]+?[\s*]+)(gpp_\w+)\s*\(([^()]*)\)\s*;', text):
        result = ' '.join(result.replace('*', ' * ').split())
        assert result in ('int', 'const char *'), '{}: result {!r}'.format(name, result)
        classes = []
        for p in ([] if params.strip() in ('', 'void') else params.split(',')):
            if '*' in p or '[' in p:
                classes.append('pointer')
                continue
            words = [w for w in p.split() if w != 'const']
            kind = ' '.join(words[:-1])                     # the last word is the parameter's name
            assert kind in C_CLASS, '{}: parameter {!r} is of no known class'.format(name, ' '.join(p.split()))
            classes.append(C_CLASS[kind])
        assert name not in found, '{} is declared twice'.format(name)
        found[name] = ('pointer' if '*' in result else 'int32', classes)
    named = set(re.findall(r'\b(gpp_\w+)\s*\(', text))
    assert named == set(found), 'prototypes the parser did not take: {}'.format(sorted(named ^ set(found)))
    return found


def ctypes_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return 'pointer'
    return CTYPES_CLASS[t]


class EveryEntryPoint(object):
    """ stands in for the loaded library: it has every gpp_* attribute, so _declare opens every gate """
    class Function(object):
        pass

    def __getattr__(self, name):
        if not name.startswith('gpp_'):
            raise AttributeError(name)
        return self.__dict__.setdefault(name, self.Function())


def test_signatures():
    """ every function the header declares is bound, nothing else is, and each argument list is the prototype's: the count and, per
    parameter, the class (pointer, int32, uint32, size_t, float, double, int64) """
    declared = prototypes()
    assert len(declared) >= 104
    lib = EveryEntryPoint()
    hip._declare(lib)
    bound = {n: f for n, f in vars(lib).items() if hasattr(f, 'argtypes')}
    wrong = ['{} is declared in the header and not bound'.format(n) for n in sorted(set(declared) - set(bound))]
    wrong += ['{} is bound and not declared in the header'.format(n) for n in sorted(set(bound) - set(declared))]
    for name in sorted(set(bound) & set(declared)):
        got = (ctypes_class(bound[name].restype), [ctypes_class(t) for t in bound[name].argtypes])
        if got != declared[name]:
            wrong.append('{}: bound as {}, declared as {}'.format(name, got, declared[name]))
    assert not wrong, '\n'.join(wrong)
