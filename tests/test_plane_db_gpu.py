""" The plane distillation on the GPU (csrc/plane_db.hip): the cost table against the functions of oracle/polling_np.py
composed with the key formula, its agreement with gpp_poll_f32's own choice, gpp_plane_select against utils/plane_db.select_np and the
loop-written oracle, and the whole path labels -> table -> picks -> .mat -> polling.

Every comparison is for equality: the table's float32 steps are those of the polling kernel (bit-exact against the oracle), the
selection is integer arithmetic. """
import ctypes
import os

import numpy as np
import pytest
import torch

import label_prep_oracle as LO
import plane_db_oracle as PO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.bin import distil_planes
from keras_retinanet_3D.utils import gpp_utils, plane_db, synthetic
from keras_retinanet_3D.utils import label_prep as L

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------- the cost table
SEED = 11             # chosen on the CPU: with it oracle/polling_np.py alone shows 8 of the 9 non-padding rows (89 %) below residual 16
M_MAX = 1031
SIZES = [1, 255, 256, 257, 1031]
PAD_ROW, NAN_ROW = (1, 4), (0, 2)
FILL = 0x5a5a


def polling_inputs(seed=SEED):
    """ B = 2 images of D = 5 detections on rows of the pool; one -1 padding row, one row whose top keypoint is NaN (a NaN residual).
    The pool: 600 rows of the shipped 22k database, then seeded planes of every attitude -- steep ones put an object's corners behind
    each other (zc < 0), low ones miss by metres (fewer than six votes, a residual sum beyond 8 m) """
    rng = np.random.default_rng(seed)
    road = synthetic.load_plane_database('22k')[:600]
    normals = rng.normal(size=(M_MAX - 600, 3)) * np.array([1.0, 0.6, 1.0])
    wild = np.concatenate([normals, rng.uniform(-12.0, 12.0, size=(M_MAX - 600, 1))], axis=1)
    pool = np.concatenate([road, wild])[rng.permutation(M_MAX)].astype(np.float32)
    pool[0] = road[0]                                        # M = 1: a plane of the road
    inp = synthetic.synthetic_polling_batch(pool[:256].astype(np.float64), batch=2, num_dets=5, seed=seed)
    boxes, dims, orient = inp['boxes'].copy(), inp['dimensions'].copy(), inp['orientations'].copy()
    boxes[PAD_ROW], dims[PAD_ROW], orient[PAD_ROW] = -1.0, -1.0, -1
    boxes[NAN_ROW][10] = np.nan
    return {'boxes': boxes, 'dims': dims, 'orient': orient, 'P_inv': inp['P_inv'], 'pool': pool}


@pytest.fixture(scope='module')
def costs():
    inp = polling_inputs()
    keys, votes, res, zc = PO.cost_keys(inp['boxes'], inp['dims'], inp['orient'], inp['P_inv'], inp['pool'])
    live = np.ones(10, bool)
    live[PAD_ROW[0] * 5 + PAD_ROW[1]] = False
    # the table has what it is meant to have
    assert (keys[~live] == 65535).all() and (keys[NAN_ROW[0] * 5 + NAN_ROW[1]] == 65535).all() and np.isnan(res[NAN_ROW[0] * 5 + NAN_ROW[1]]).all()
    ok = live.copy()
    ok[NAN_ROW[0] * 5 + NAN_ROW[1]] = False
    with np.errstate(invalid='ignore'):
        assert (zc[ok] < 0).any() and (keys[ok][zc[ok] < 0] == 65535).all()
        valid = keys[ok] != 65535
        assert (votes[ok][valid] < 6).any() and (votes[ok][valid] == 6).any() and (res[ok][valid] > 8.0).any()
    assert ((keys[ok][valid] & 8191) == 8191).any() and keys[ok][valid].max() <= 57343 and keys[ok].min() < 8192
    dev = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    return dict(inp, keys=keys, live=live, dev=dev)


def run_costs(c, M, images=slice(None), pitch=None, row_index=None, row_offset=0, table=None, rows=None):
    d = c['dev']
    pitch = hip.table_pitch(M) if pitch is None else pitch
    n = len(row_index) if row_index is not None else int(d['orient'][images].numel())
    if table is None:
        table = torch.full((n + row_offset if rows is None else rows, pitch), FILL, dtype=torch.int16, device='cuda')
    index = None if row_index is None else torch.as_tensor(np.asarray(row_index, np.int32)).cuda()
    done = hip.poll_costs(d['boxes'][images].contiguous(), d['dims'][images].contiguous(), d['orient'][images].contiguous(),
                          d['P_inv'][images].contiguous(), d['pool'][:M].contiguous(), table, index, row_offset)
    torch.cuda.synchronize()
    assert done == n
    return table


def as_keys(table):
    return table.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('M', SIZES)
def test_cost_table_equals_the_oracle(costs, M):
    got = as_keys(run_costs(costs, M))
    assert got.shape == (10, hip.table_pitch(M)) and np.array_equal(got[:, :M], costs['keys'][:, :M])
    assert (got[:, M:] == FILL).all()


@pytest.mark.parametrize('M', [257, 1031])
def test_cost_table_of_listed_rows_with_a_wider_pitch(costs, M):
    rows = [7, 2, 9, 0, 7]                                   # any order, the padding row, one row twice
    pitch = hip.table_pitch(M) + 16
    got = as_keys(run_costs(costs, M, pitch=pitch, row_index=rows, row_offset=2, rows=9))
    assert np.array_equal(got[2:7, :M], costs['keys'][rows, :M])
    assert (got[2:7, M:] == FILL).all() and (got[:2] == FILL).all() and (got[7:] == FILL).all()


def test_two_chunks_fill_one_table(costs):
    M = 257
    table = run_costs(costs, M, images=slice(0, 1), rows=10)
    table = run_costs(costs, M, images=slice(1, 2), row_offset=5, table=table)
    got = as_keys(table)
    assert np.array_equal(got[:, :M], costs['keys'][:, :M]) and (got[:, M:] == FILL).all()


def test_cost_table_argument_errors_launch_nothing(costs):
    d, M = costs['dev'], 256
    lib = hip.lib()
    table = torch.full((10, 264), FILL, dtype=torch.int16, device='cuda')
    work = torch.empty((16 * M + 16,), dtype=torch.uint8, device='cuda')
    pool = d['pool'][:M].contiguous()

    def call(planes=pool, pitch=264, tab=table.data_ptr(), wbytes=16 * M, wptr=work.data_ptr(), O=10, offset=0):
        return lib.gpp_poll_costs_u16(hip.ptr(d['boxes']), hip.ptr(d['dims']), hip.ptr(d['orient']), hip.ptr(d['P_inv']), hip.ptr(planes), 2, 5, M,
                                      0.7, None, O, ctypes.c_void_p(tab), pitch, offset, ctypes.c_void_p(wptr), wbytes, hip.stream_ptr())
    assert call(pitch=255) == -1 and call(pitch=260) == -1 and call(O=9) == -1 and call(offset=-1) == -1 and call(tab=None) == -1
    assert call(wbytes=16 * M - 1) == -2
    assert call(tab=table.data_ptr() + 2) == -3 and call(wptr=work.data_ptr() + 8) == -3
    torch.cuda.synchronize()
    assert (as_keys(table) == FILL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(as_keys(table)[:, :M], costs['keys'][:, :M])


def test_the_plane_polling_picks_has_the_smallest_key(costs):
    """ the key is monotone in polling's own order (votes, then the residual among planes with zc >= 0): wherever polling's winner is no
    sentinel (residual below 16 -- the sentinel is 100 / 6), its key is the row's minimum """
    d = costs['dev']
    _, _, residuals, index = gpp_utils.fit_road_planes(d['boxes'], d['dims'], d['orient'], d['P_inv'], d['pool'], return_index=True)
    residuals, index = residuals.cpu().numpy().reshape(-1), index.cpu().numpy().reshape(-1)
    keys = costs['keys']
    with np.errstate(invalid='ignore'):
        qualifies = costs['live'] & (residuals < 16.0)
    print('rows below residual 16: {} of {} non-padding rows'.format(int(qualifies.sum()), int(costs['live'].sum())))
    assert qualifies.sum() >= 0.8 * costs['live'].sum()
    for o in np.nonzero(qualifies)[0]:
        assert keys[o, index[o]] == keys[o].min(), o
    got = as_keys(run_costs(costs, M_MAX))[:, :M_MAX]
    for o in np.nonzero(qualifies)[0]:
        assert got[o, index[o]] == got[o].min(), o


# ---------------------------------------------------------------------------------------------------- the selection
def run_select(table, K, extra_pitch=0):
    """ table (O, M) uint16 -> the dict of select_np, from gpp_plane_select on an upload whose pad columns hold zeros (the most tempting
    garbage: a pad column that counted would win every pick) """
    O, M = table.shape
    padded = np.zeros((O, hip.table_pitch(M) + extra_pitch), np.uint16)
    padded[:, :M] = table
    return plane_db.select(torch.as_tensor(padded.view(np.int16)).cuda(), M, K)


def same(got, want):
    for name in ('chosen', 'trace', 'best'):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert got['count'] == want['count']


@pytest.mark.parametrize('M', [1, 255, 256, 257, 2049])
@pytest.mark.parametrize('O', [1, 63, 64, 65, 1000])
def test_select_equals_select_np(O, M):
    table = PO.seeded_table(7000 * O + M, O, M)
    K = min(M, 40)
    got, want = run_select(table, K, extra_pitch=8 if M == 257 else 0), plane_db.select_np(table, K)
    same(got, want)
    if O * M * K <= 700000:
        chosen, trace, best, count = PO.select_loops(table, K)
        assert got['chosen'].tolist() == chosen and [int(v) for v in got['trace']] == trace and got['best'].tolist() == best and got['count'] == count
    PO.check_result(table, K, got['chosen'], got['trace'], got['best'], got['count'])


def test_select_duplicate_columns_no_valid_pair_and_exhaustion():
    table = PO.seeded_table(5, 37, 7)
    table[:, 1] = 65535
    table[:, 4] = np.minimum(table[:, 4], 3000)
    table[:, 2] = table[:, 4]
    got = run_select(table, 7)
    same(got, plane_db.select_np(table, 7))
    assert got['chosen'][0] == 2 and 4 not in got['chosen'].tolist() and 1 not in got['chosen'].tolist() and got['count'] < 7
    assert int(got['trace'][-1]) == int(table.min(axis=1).astype(np.int64).sum())

    nothing = np.full((65, 300), 65535, np.uint16)
    got = run_select(nothing, 5)
    same(got, plane_db.select_np(nothing, 5))
    assert got['count'] == 0 and got['chosen'].tolist() == [-1] * 5 and got['trace'].tolist() == [65535 * 65] * 6

    table = PO.seeded_table(78, 37, 300)
    got = run_select(table, 300)
    same(got, plane_db.select_np(table, 300))
    assert got['count'] < 300 and int(got['trace'][-1]) == int(table.min(axis=1).astype(np.int64).sum())


def test_select_sums_a_gain_beyond_32_bits():
    table = PO.seeded_table(3, 70000, 8, special=False)
    table[:, 5] = 0
    got = run_select(table, 8)
    assert got['chosen'][0] == 5 and int(got['trace'][0]) - int(got['trace'][1]) == 70000 * 65535 > 2 ** 32
    assert got['count'] == 1 and int(got['trace'][-1]) == 0
    table[::2, 5] = 65535                                    # half the rows: the other planes still gain after it
    got = run_select(table, 8)
    same(got, plane_db.select_np(table, 8))
    assert got['count'] > 1


def test_select_argument_errors_launch_nothing():
    lib = hip.lib()
    table = torch.zeros((8, 16), dtype=torch.int16, device='cuda')
    chosen = torch.full((20,), 7, dtype=torch.int32, device='cuda')
    trace = torch.full((21,), 7, dtype=torch.int64, device='cuda')
    best = torch.full((8,), 7, dtype=torch.int16, device='cuda')
    count = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    work = torch.empty((8 * 16 + 32,), dtype=torch.uint8, device='cuda')

    def call(M=12, pitch=16, K=4, O=8, wbytes=8 * 12 + 16, tab=table.data_ptr(), cnt=count.data_ptr()):
        return lib.gpp_plane_select(ctypes.c_void_p(tab), O, M, pitch, K, hip.ptr(chosen), hip.ptr(trace), hip.ptr(best), ctypes.c_void_p(cnt),
                                    hip.ptr(work), wbytes, hip.stream_ptr())
    assert call(K=13) == -1 and call(K=0) == -1 and call(M=0) == -1 and call(O=0) == -1 and call(pitch=12) == -1 and call(M=17) == -1
    assert call(cnt=None) == -1 and call(wbytes=8 * 12 + 15) == -2 and call(tab=table.data_ptr() + 8) == -3
    torch.cuda.synchronize()
    assert (chosen == 7).all() and (trace == 7).all() and (best == 7).all() and (count == 7).all()
    with pytest.raises(ValueError):
        hip.plane_select(table, 12, 13)


# ---------------------------------------------------------------------------------------------------- end to end
def own_plane_scenes():
    """ five images of eight Cars, each on a horizontal plane of its own: y = 1.30, 1.32 ... 2.08 """
    scenes, planes = [], []
    for b, seed in enumerate((31, 32, 33, 34, 35)):
        labels, P = LO.seeded_scene(seed, 8, P_offset=False, kinds=(0,), behind=0.0)
        labels[:, 12] = 1.30 + 0.02 * (8 * b + np.arange(8))
        planes += [[0.0, -1.0, 0.0, t] for t in labels[:, 12]]
        scenes.append((['Car'] * 8, labels, P))
    return scenes, np.array(planes, np.float64)


@pytest.fixture(scope='module')
def pool_and_scenes():
    scenes, own = own_plane_scenes()
    rng = np.random.default_rng(4)
    distractors = np.stack([rng.normal(0.0, 0.05, 200), -np.ones(200), rng.normal(0.0, 0.05, 200), rng.uniform(0.5, 4.0, 200)], axis=1)
    pool = np.concatenate([own, distractors])[rng.permutation(240)]
    return scenes, pool


def test_distil_rows_end_to_end(pool_and_scenes, tmp_path):
    scenes, pool = pool_and_scenes
    labels_list, P_list = [g for _, g, _ in scenes], [P for _, _, P in scenes]
    _, det = L.prepare_batch(np.stack(labels_list), [8] * 5, np.stack(P_list), det_types=L.CAR)
    objects = int((det[4] >= 0).sum())
    assert objects >= 30                                     # (all 40, unless a seeded object lies behind the camera)
    table, M = plane_db.cost_table(labels_list, P_list, pool)
    keys = table.cpu().numpy().view(np.uint16)
    assert M == 240 and keys.shape == (objects, 240)
    whole = plane_db.distil_rows(labels_list, P_list, pool, 240, report=True)
    assert whole['objects'] == objects and 1 <= whole['count'] <= 240
    assert int(whole['trace'][-1]) == int(keys.min(axis=1).astype(np.int64).sum())
    PO.check_result(keys, 240, np.concatenate([whole['indices'], -np.ones(240 - whole['count'], np.int32)]), whole['trace'], whole['best'], whole['count'])
    assert whole['planes'].dtype == pool.dtype and np.array_equal(whole['planes'], pool[whole['indices']])
    assert whole['six_vote_share'] == 1.0 and whole['served'] == objects       # every object's own plane is in the pool
    assert sorted(whole['prefixes']) == [n for n in (1, 10, 100) if n < whole['count']]
    # the two chunkings and the host selection give the same run
    chunked = plane_db.distil_rows(labels_list, P_list, pool, 240, chunk_images=2)
    host = plane_db.distil_rows(labels_list, P_list, pool, 240, device=False)
    for other in (chunked, host):
        assert np.array_equal(other['indices'], whole['indices']) and np.array_equal(other['trace'], whole['trace']) and np.array_equal(other['best'], whole['best'])
    twenty = plane_db.distil_rows(labels_list, P_list, pool, 20)
    n = min(20, whole['count'])
    assert twenty['count'] == n and np.array_equal(twenty['indices'], whole['indices'][:n]) and np.array_equal(twenty['planes'], whole['planes'][:n])
    assert np.array_equal(twenty['trace'][:n + 1], whole['trace'][:n + 1])
    # written, re-read, polled
    path = os.path.join(str(tmp_path), 'distilled.mat')
    plane_db.write_database(path, whole['planes'])
    planes = L._load_planes(path)
    assert np.array_equal(planes, whole['planes'].astype(np.float32))
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    pinv = np.stack([np.linalg.pinv(P) for P in P_list]).astype(np.float32)
    _, _, residuals, index = gpp_utils.fit_road_planes(up(det[0]), up(det[1]), up(det[4]), up(pinv), up(planes), return_index=True)
    residuals, index = residuals.cpu().numpy(), index.cpu().numpy()
    served = det[4] >= 0
    assert (index >= 0).all() and (index < planes.shape[0]).all() and (residuals[served] < 0.7).all()


def test_distil_planes_command_line(pool_and_scenes, tmp_path, capsys):
    import scipy.io
    scenes, pool = pool_and_scenes
    label_dir, calib_dir = LO.write_dataset(tmp_path, scenes)
    pool_path, out = os.path.join(str(tmp_path), 'pool.mat'), os.path.join(str(tmp_path), 'out.mat')
    plane_db.write_database(pool_path, pool)
    result = distil_planes.main([label_dir, calib_dir, pool_path, out, '--planes', '30', '--report'])
    lines = capsys.readouterr().out.splitlines()
    sizes = plane_db.prefix_sizes(result['count'])
    assert len(lines) == len(sizes) + 1 and all('six votes' in line for line in lines[:-1])
    assert [int(line.split()[0]) for line in lines[:-1]] == sizes
    written = scipy.io.loadmat(out)['road_planes_database']
    assert written.shape == (result['count'], 4) and np.array_equal(written, pool[result['indices']])
    again = plane_db.distil(label_dir, calib_dir, pool_path, 30)
    assert np.array_equal(again['indices'], result['indices'])
