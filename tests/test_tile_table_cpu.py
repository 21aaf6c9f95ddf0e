"""
The convolution's tile catalogue (csrc/conv_tiles.h) as a truth table, without a device.

gpp_conv2d_igemm on a well-formed descriptor answers, BEFORE any launch, one of three things when no device is visible: GPP_ERR_BAD_ARG (the
tile code is in nobody's table), GPP_ERR_UNSUPPORTED (the code exists, this element type / input form / layer cannot run it) or a positive
hipError_t (every check passed: it would have launched).  tests/golden/tile_table.json holds, for a set of layers crossed with the element
types and the x3 input forms,

  * the ordered answer of gpp_conv2d_tile_candidates / gpp_conv2d_preact_tile_candidates (the autotuner's strict `<` lets the order decide ties),
  * the class (-1, -4, "> 0" written as 1; any other negative code as itself) of the return code for every catalogue code, every such code
    +- 1, 0, the legacy codes, the retired 3064128 and every integer below 300 000,
  * the candidates that the same descriptor then refuses (`refused`: a candidate the dispatcher rejects is a tile the tuner times in vain).

The file was written by `python tests/test_tile_table_cpu.py --write` from the library as it was BEFORE the catalogue moved into one table
(hand-kept switch, list and predicate): the table has to reproduce it exactly.

Pinned findings, kept as they were (`refused` of the golden file; the tuner skips a tile that is refused):
  * on an x3 type with a float32 (not pre-split) input map, the candidate list of the 144-channel layer names 192160, which such a type has
    on pre-split input only: dispatch answers GPP_ERR_UNSUPPORTED;
  * the mixed-height grid 3256224 is listed for the 512 -> 512 head layer (its hard conditions hold) and refused by the launcher, whose cost
    model finds no split that beats the uniform grid;
  * the 16-bit types answer GPP_ERR_BAD_ARG, not GPP_ERR_UNSUPPORTED, to the codes only the x3 types have.

The work runs in a child process that sees no device (HIP_VISIBLE_DEVICES=-1, ROCR_VISIBLE_DEVICES empty) and checks so first: with a device
a runnable tile would really be launched, on made-up pointers.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'tile_table.json')
SWEEP = 300000

# every code the catalogue has held (the pin of this test, not a second catalogue: the library is asked about each of them)
CODES = [64, 128, 256, 512, 3064128,
         64064, 96064, 128064, 160064, 192064, 64128, 96128, 128128, 160128, 192128, 224128,
         1128128, 1192128, 1128256, 1160256, 1192256, 1224256, 256256, 1256256,
         128160, 192160, 1192160, 1128160, 2256256, 1192096, 3256224, 3192160, 4128064, 4064064, 4128128, 4064128,
         5064064, 5096064, 5064128, 5096128, 5128128, 128256, 192256,
         6064064, 6032064, 6064160, 7064064, 7032064, 7064160]
DTYPES = (1, 2, 3, 4, 5)              # GPP_BF16, GPP_F16, GPP_F32, GPP_BF16X3, GPP_F16X3
X3_IN, X3_OUT, X3_RES = 1, 2, 4
PYRAMID = [(48, 72), (24, 36), (12, 18), (6, 9), (3, 5)]
# name -> (entry point, k, C_in, C_out, batch, maps, shortcut, out_f32, workspace, gathered)
LAYERS = {
    'head_512_512': ('igemm', 3, 512, 512, 8, PYRAMID, False, False, False, False),          # 256-column tiles, mix grids
    'head_512_896': ('igemm', 3, 512, 896, 8, PYRAMID, False, False, False, False),          # dual grid: C_out = 256 k + 128
    'head_512_144_f32out': ('igemm', 3, 512, 144, 8, PYRAMID, False, True, False, False),    # 160-column tiles
    'head_512_96_f32out': ('igemm', 3, 512, 96, 8, PYRAMID, False, True, False, False),      # 96-column tiles
    'c1x1_128_512_shortcut': ('igemm', 1, 128, 512, 2, [(48, 48)], True, False, False, False),   # weight-stationary: all four tiles
    'c1x1_512_128': ('igemm', 1, 512, 128, 2, [(48, 48)], False, False, False, False),       # weight-stationary: the 64-row ring only
    'c1x1_64_256': ('igemm', 1, 64, 256, 2, [(48, 48)], False, False, False, False),         # shallow: narrow tiles on a wide layer
    'p5_512_512': ('igemm', 3, 512, 512, 1, [(12, 39)], False, False, False, False),         # deep-ring tiles
    'p5_512_512_workspace': ('igemm', 3, 512, 512, 1, [(12, 39)], False, False, True, False),    # ... and the split rule at work
    'gather_512_144': ('igemm', 3, 512, 144, 8, PYRAMID, False, True, False, True),
    'gather_512_96': ('igemm', 3, 512, 96, 8, PYRAMID, False, True, False, True),
    'preact_256_128': ('preact', 1, 256, 128, 2, [(48, 48)], False, False, False, False),
}


def cases():
    for name in LAYERS:
        for dt in DTYPES:
            for x3 in ((0, X3_IN, X3_IN | X3_OUT | X3_RES) if dt >= 4 else (0,)):
                yield name, dt, x3


def make_desc(hip, name, dt, x3):
    _, k, cin, cout, batch, maps, res, out_f32, workspace, gathered = LAYERS[name]
    d = hip.ConvDesc()
    d.inp, d.weight, d.out, d.bias, d.zero_page = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    if res:
        d.residual, d.res_pitch = 0x600000, cout
    if workspace:
        d.partial, d.partial_bytes = 0x700000, 1 << 30
    if gathered:
        d.gather_rows, d.gather_counts = 0x800000, 0x900000
    if dt == hip.GPP_F16X3:
        d.range_counter = 0xa00008          # (without one, and without a device, the entry point gives up before it dispatches)
    d.dtype, d.out_f32, d.batch, d.C_in, d.C_out, d.KH, d.KW, d.stride = dt, int(out_f32), batch, cin, cout, k, k, 1
    d.pad_top = d.pad_left = k // 2
    d.in_pitch, d.out_pitch, d.weight_rows, d.n_groups, d.x3_split = cin, cout, (cout + 255) // 256 * 256, len(maps), x3
    off = 0
    for g, (h, w) in enumerate(maps):
        G = d.groups[g]
        G.H_in, G.W_in, G.H_out, G.W_out, G.H_res, G.W_res = h, w, h, w, h, w
        G.in_off, G.out_off, G.res_off = off * cin, off * cout, off * cout
        G.in_bstride, G.out_bstride, G.res_bstride = h * w * cin, h * w * cout, h * w * cout
        off += batch * h * w
    return d


def klass(rc):
    return 1 if rc > 0 else rc


def probe_one(index):
    from keras_retinanet_3D.backend import hip
    lib = hip.lib()
    name, dt, x3 = list(cases())[index]
    d = make_desc(hip, name, dt, x3)
    ref = ctypes.byref(d)
    if LAYERS[name][0] == 'preact':
        table = (ctypes.c_float * 1024)()
        scale = (ctypes.addressof(table) + 15) // 16 * 16         # (never read: no launch happens)
        lib.gpp_conv2d_preact.restype = ctypes.c_int
        lib.gpp_conv2d_preact.argtypes = [ctypes.POINTER(hip.ConvDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        run = lambda: lib.gpp_conv2d_preact(ref, scale, scale + 2048, None)  # noqa: E731
        listing = lib.gpp_conv2d_preact_tile_candidates
    else:
        run = lambda: lib.gpp_conv2d_igemm(ref, None)  # noqa: E731
        listing = lib.gpp_conv2d_tile_candidates
    tiles, count = (ctypes.c_int * 128)(), ctypes.c_int(0)
    rc = listing(ref, tiles, 128, ctypes.byref(count))
    candidates = list(tiles[:count.value]) if rc == 0 else rc
    probes = sorted(set(range(SWEEP)) | {c + s for c in CODES for s in (-1, 0, 1)})
    answers = {}
    for code in probes:
        d.tile_hint = code
        answers[code] = klass(run())
    # compact form: the class of the great majority, and the codes that answer otherwise
    values = list(answers.values())
    common = max(set(values), key=values.count)
    refused = [c for c in candidates if answers[c] != 1] if rc == 0 else []
    return {'case': '{}/dtype{}/x3_split{}'.format(name, dt, x3), 'candidates': candidates, 'common': common,
            'codes': {str(c): v for c, v in answers.items() if v != common}, 'refused': refused}


def child():
    sys.path.insert(0, os.path.join(ROOT, 'ground-plane-polling_amd'))
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() > 0:
        print(json.dumps({'skip': 'a device is visible in the child'}))
        return
    import multiprocessing
    n = len(list(cases()))
    with multiprocessing.get_context('fork').Pool(min(8, os.cpu_count() or 1)) as pool:
        rows = pool.map(probe_one, range(n), chunksize=1)
    print(json.dumps({'rows': rows}))


def run_child():
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_catalogue_answers_as_the_golden_table():
    got = run_child()
    if 'skip' in got:
        pytest.skip(got['skip'])
    with open(GOLDEN) as f:
        want = json.load(f)
    assert [r['case'] for r in got['rows']] == [r['case'] for r in want['rows']]
    for g, w in zip(got['rows'], want['rows']):
        assert g['candidates'] == w['candidates'], g['case']
        assert g['common'] == w['common'], g['case']
        assert g['codes'] == w['codes'], (g['case'], sorted(set(g['codes'].items()) ^ set(w['codes'].items())))
        # every candidate is runnable on its own descriptor -- but for the pinned findings of the module docstring
        assert g['refused'] == w['refused'], g['case']
        assert set(g['refused']) <= {192160, 3256224}, g['case']
    # the set is not vacuous: something runs, something is refused, something is unknown, in every entry point
    flat = [v for r in got['rows'] for v in list(r['codes'].values()) + [r['common']]]
    assert {1, -1, -4} <= set(flat)
    assert any(r['candidates'] != 0 and len(r['candidates']) > 10 for r in got['rows'] if isinstance(r['candidates'], list))


if __name__ == '__main__':
    if '--child' in sys.argv:
        child()
    elif '--write' in sys.argv:
        out = run_child()
        assert 'rows' in out, out
        with open(GOLDEN, 'w') as f:
            json.dump(out, f, separators=(',', ':'))
            f.write('\n')
        print('wrote', GOLDEN, len(out['rows']), 'rows')
