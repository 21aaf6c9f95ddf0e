""" The distillation for the polled location error on the GPU (csrc/plane_db.hip, csrc/pose_eval.h): gpp_pose_costs_u16
against gpp_poll_costs_u16 and utils/plane_db.pair_costs_np, gpp_plane_select_polled against select_polled_np and the loop-written
oracle, and the whole path labels -> two tables -> picks -> .mat -> polling.

Every comparison is for equality: the tables' float32 steps are separate operations in one order on both sides, the selection is
integer arithmetic. """
import ctypes
import os

import numpy as np
import pytest
import torch

import label_prep_oracle as LO
import plane_db_location_oracle as QO
from keras_retinanet_3D.backend import hip
from keras_retinanet_3D.bin import distil_planes
from keras_retinanet_3D.utils import gpp_utils, plane_db
from keras_retinanet_3D.utils import label_prep as L

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1031]
FILL = 0x5a5a


# ---------------------------------------------------------------------------------------------------- the cost tables
@pytest.fixture(scope='module')
def costs():
    inp = QO.polling_inputs()
    keys, errs = plane_db.pair_costs_np(inp['boxes'], inp['dims'], inp['orient'], inp['P_inv'], inp['want'], inp['pool'])
    pad, nan = QO.PAD_ROW[0] * 5 + QO.PAD_ROW[1], QO.NAN_ROW[0] * 5 + QO.NAN_ROW[1]
    assert (keys[pad] == 65535).all() and (keys[nan] == 65535).all() and ((errs == 65535) == (keys == 65535)).all()
    assert 0.05 < (keys == 65535).mean() < 0.95 and errs[keys != 65535].max() == 65534 and errs.min() < 256
    dev = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    return dict(inp, keys=keys, errs=errs, dev=dev)


def run_costs(c, M, images=slice(None), pitch=None, row_index=None, row_offset=0, tables=None, rows=None):
    d = c['dev']
    pitch = hip.table_pitch(M) if pitch is None else pitch
    n = len(row_index) if row_index is not None else int(d['orient'][images].numel())
    if tables is None:
        shape = (n + row_offset if rows is None else rows, pitch)
        tables = (torch.full(shape, FILL, dtype=torch.int16, device='cuda'), torch.full(shape, FILL, dtype=torch.int16, device='cuda'))
    index = None if row_index is None else torch.as_tensor(np.asarray(row_index, np.int32)).cuda()
    done = hip.pose_costs(d['boxes'][images].contiguous(), d['dims'][images].contiguous(), d['orient'][images].contiguous(),
                          d['P_inv'][images].contiguous(), d['want'][images].contiguous(), d['pool'][:M].contiguous(), tables[0], tables[1],
                          index, row_offset)
    torch.cuda.synchronize()
    assert done == n
    return tables


def u16(table):
    return table.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('M', SIZES)
def test_both_tables_equal_the_numpy_form_and_the_keys_equal_poll_costs(costs, M):
    keys_t, errs_t = run_costs(costs, M)
    d = costs['dev']
    old = torch.full(tuple(keys_t.shape), FILL, dtype=torch.int16, device='cuda')
    hip.poll_costs(d['boxes'], d['dims'], d['orient'], d['P_inv'], d['pool'][:M].contiguous(), old)
    torch.cuda.synchronize()
    keys, errs = u16(keys_t), u16(errs_t)
    assert keys.shape == (10, hip.table_pitch(M)) and np.array_equal(keys, u16(old))
    assert np.array_equal(keys[:, :M], costs['keys'][:, :M]) and np.array_equal(errs[:, :M], costs['errs'][:, :M])
    assert (keys[:, M:] == FILL).all() and (errs[:, M:] == FILL).all()


@pytest.mark.parametrize('M', [257, 1031])
def test_tables_of_listed_rows_with_a_wider_pitch(costs, M):
    rows = [7, 2, 9, 0, 7]                                   # any order, the padding row, one row twice
    pitch = hip.table_pitch(M) + 16
    keys_t, errs_t = run_costs(costs, M, pitch=pitch, row_index=rows, row_offset=2, rows=9)
    for got, want in ((u16(keys_t), costs['keys']), (u16(errs_t), costs['errs'])):
        assert np.array_equal(got[2:7, :M], want[rows, :M])
        assert (got[2:7, M:] == FILL).all() and (got[:2] == FILL).all() and (got[7:] == FILL).all()


def test_a_list_entry_outside_the_batch_is_invalid_throughout(costs):
    keys_t, errs_t = run_costs(costs, 257, row_index=[3, 10, -1, 0])
    keys, errs = u16(keys_t), u16(errs_t)
    assert (keys[1:3, :257] == 65535).all() and (errs[1:3, :257] == 65535).all()
    assert np.array_equal(errs[[0, 3], :257], costs['errs'][[3, 0], :257]) and np.array_equal(keys[[0, 3], :257], costs['keys'][[3, 0], :257])


def test_two_chunks_fill_one_pair_of_tables(costs):
    M = 257
    tables = run_costs(costs, M, images=slice(0, 1), rows=10)
    tables = run_costs(costs, M, images=slice(1, 2), row_offset=5, tables=tables)
    for got, want in ((u16(tables[0]), costs['keys']), (u16(tables[1]), costs['errs'])):
        assert np.array_equal(got[:, :M], want[:, :M]) and (got[:, M:] == FILL).all()


def test_pose_costs_argument_errors_launch_nothing(costs):
    d, M = costs['dev'], 256
    lib = hip.lib()
    keys = torch.full((10, 264), FILL, dtype=torch.int16, device='cuda')
    errs = torch.full((10, 264), FILL, dtype=torch.int16, device='cuda')
    work = torch.empty((16 * M + 16,), dtype=torch.uint8, device='cuda')
    pool = d['pool'][:M].contiguous()

    def call(pitch=264, kt=keys.data_ptr(), et=errs.data_ptr(), wbytes=16 * M, wptr=work.data_ptr(), O=10, offset=0, want=d['want'].data_ptr(),
             planes=pool.data_ptr()):
        return lib.gpp_pose_costs_u16(hip.ptr(d['boxes']), hip.ptr(d['dims']), hip.ptr(d['orient']), hip.ptr(d['P_inv']), ctypes.c_void_p(want),
                                      ctypes.c_void_p(planes), 2, 5, M, 0.7, None, O, ctypes.c_void_p(kt), ctypes.c_void_p(et), pitch, offset,
                                      ctypes.c_void_p(wptr), wbytes, hip.stream_ptr())
    assert call(pitch=255) == -1 and call(pitch=260) == -1 and call(O=9) == -1 and call(offset=-1) == -1
    assert call(kt=None) == -1 and call(et=None) == -1 and call(want=None) == -1 and call(wptr=None) == -1
    assert call(wbytes=16 * M - 1) == -2
    assert call(kt=keys.data_ptr() + 2) == -3 and call(et=errs.data_ptr() + 8) == -3 and call(wptr=work.data_ptr() + 8) == -3
    assert call(planes=pool.data_ptr() + 4) == -3
    torch.cuda.synchronize()
    assert (u16(keys) == FILL).all() and (u16(errs) == FILL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(u16(keys)[:, :M], costs['keys'][:, :M]) and np.array_equal(u16(errs)[:, :M], costs['errs'][:, :M])
    with pytest.raises(ValueError):
        hip.pose_costs(d['boxes'], d['dims'], d['orient'], d['P_inv'], d['want'][:, :, :2].contiguous(), pool, keys, errs)


# ---------------------------------------------------------------------------------------------------- the selection
def run_select(keys, errs, K, extra_pitch=0):
    """ (O, M) uint16 tables -> the dict of select_polled_np, from gpp_plane_select_polled on uploads whose pad columns hold zeros (the
    most tempting garbage: a pad column of key 0 and error 0 that counted would win the first pick) """
    O, M = keys.shape
    up = []
    for t in (keys, errs):
        padded = np.zeros((O, hip.table_pitch(M) + extra_pitch), np.uint16)
        padded[:, :M] = t
        up.append(torch.as_tensor(padded.view(np.int16)).cuda())
    return plane_db.select_polled(up[0], up[1], M, K)


def same(got, want):
    for name in ('chosen', 'trace', 'best', 'cur'):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert got['count'] == want['count']


@pytest.mark.parametrize('M', [1, 255, 256, 257, 2049])
@pytest.mark.parametrize('O', [1, 63, 64, 65, 1000])
def test_select_polled_equals_select_polled_np(O, M):
    keys, errs = QO.seeded_pair(7000 * O + M, O, M)
    K = min(M, 40)
    got, want = run_select(keys, errs, K, extra_pitch=8 if M == 257 else 0), plane_db.select_polled_np(keys, errs, K)
    same(got, want)
    if O * M * K <= 700000:
        chosen, trace, best, cur, count = QO.select_polled_loops(keys, errs, K)
        assert got['chosen'].tolist() == chosen and [int(v) for v in got['trace']] == trace and got['count'] == count
        assert got['best'].tolist() == best and got['cur'].tolist() == cur
        QO.check_result(keys, errs, K, got['chosen'], got['trace'], got['best'], got['cur'], got['count'])


def test_select_polled_duplicate_columns_no_valid_pair_and_exhaustion():
    keys, errs = QO.seeded_pair(5, 37, 7)
    keys[:, 1] = errs[:, 1] = 65535
    keys[:, 4], errs[:, 4] = np.minimum(keys[:, 4], 3000), np.minimum(errs[:, 4], 5)
    keys[:, 2], errs[:, 2] = keys[:, 4], errs[:, 4]
    got = run_select(keys, errs, 7)
    same(got, plane_db.select_polled_np(keys, errs, 7))
    assert got['chosen'][0] == 2 and 4 not in got['chosen'].tolist() and 1 not in got['chosen'].tolist() and got['count'] < 7

    nothing = np.full((65, 300), 65535, np.uint16)
    got = run_select(nothing, nothing, 5)
    same(got, plane_db.select_polled_np(nothing, nothing, 5))
    assert got['count'] == 0 and got['chosen'].tolist() == [-1] * 5 and got['trace'].tolist() == [65535 * 65] * 6
    assert (got['cur'] == 65535).all() and (got['best'] == 65535).all()

    keys, errs = QO.seeded_pair(78, 37, 300)                 # to exhaustion: the run ends by itself, the launches after it write -1
    got = run_select(keys, errs, 300)
    same(got, plane_db.select_polled_np(keys, errs, 300))
    assert 1 < got['count'] < 300 and (got['chosen'][got['count']:] == -1).all()
    QO.check_result(keys, errs, 300, got['chosen'], got['trace'], got['best'], got['cur'], got['count'])


def test_select_polled_sums_gains_beyond_32_bits_of_either_sign():
    O = 70000
    keys, errs = QO.seeded_pair(3, O, 8, special=False)
    keys[:, 5], errs[:, 5] = 0, 0
    got = run_select(keys, errs, 8)
    assert got['chosen'][0] == 5 and int(got['trace'][0]) - int(got['trace'][1]) == O * 65535 > 2 ** 32
    assert got['count'] == 1 and int(got['trace'][-1]) == 0 and (got['cur'] == 0).all()
    same(got, plane_db.select_polled_np(keys, errs, 8))
    # the first pick leaves cur = 0 with best = 5 > 0; column 2 then has the smaller key everywhere and the largest error: its gain is
    # -70 000 x 65534, below -2^32.  A gain that wrapped, or was compared unsigned, would be picked.
    keys[:, 5] = 5
    keys[:, 2], errs[:, 2] = 0, 65534
    got = run_select(keys, errs, 8)
    assert got['chosen'][0] == 5 and 2 not in got['chosen'].tolist() and got['count'] == 1 and (got['best'] == 5).all()
    assert O * 65534 > 2 ** 32
    same(got, plane_db.select_polled_np(keys, errs, 8))
    # half the rows: the other planes still gain after it, with terms of both signs
    keys[::2, 5] = errs[::2, 5] = 65535
    got = run_select(keys, errs, 8)
    same(got, plane_db.select_polled_np(keys, errs, 8))
    assert got['count'] > 1


def test_select_polled_argument_errors_launch_nothing():
    lib = hip.lib()
    keys = torch.zeros((8, 16), dtype=torch.int16, device='cuda')
    errs = torch.zeros((8, 16), dtype=torch.int16, device='cuda')
    chosen = torch.full((20,), 7, dtype=torch.int32, device='cuda')
    trace = torch.full((21,), 7, dtype=torch.int64, device='cuda')
    best = torch.full((8,), 7, dtype=torch.int16, device='cuda')
    cur = torch.full((8,), 7, dtype=torch.int16, device='cuda')
    count = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    work = torch.empty((8 * 16 + 32,), dtype=torch.uint8, device='cuda')
    need = ctypes.c_size_t(0)
    assert lib.gpp_plane_select_polled_workspace_bytes(12, ctypes.byref(need)) == 0 and need.value == 8 * 12 + 16
    assert lib.gpp_plane_select_polled_workspace_bytes(12, None) == -1 and lib.gpp_plane_select_polled_workspace_bytes(-1, ctypes.byref(need)) == -1

    def call(M=12, pitch=16, K=4, O=8, wbytes=8 * 12 + 16, kt=keys.data_ptr(), et=errs.data_ptr(), cnt=count.data_ptr(), cu=cur.data_ptr(),
             tr=trace.data_ptr()):
        return lib.gpp_plane_select_polled(ctypes.c_void_p(kt), ctypes.c_void_p(et), O, M, pitch, K, hip.ptr(chosen), ctypes.c_void_p(tr), hip.ptr(best),
                                           ctypes.c_void_p(cu), ctypes.c_void_p(cnt), hip.ptr(work), wbytes, hip.stream_ptr())
    assert call(K=13) == -1 and call(K=0) == -1 and call(M=0) == -1 and call(O=0) == -1 and call(pitch=12) == -1 and call(M=17) == -1
    assert call(cnt=None) == -1 and call(et=None) == -1 and call(kt=None) == -1 and call(cu=None) == -1
    assert call(wbytes=8 * 12 + 15) == -2
    assert call(kt=keys.data_ptr() + 8) == -3 and call(et=errs.data_ptr() + 8) == -3 and call(tr=trace.data_ptr() + 4) == -3
    torch.cuda.synchronize()
    assert (chosen == 7).all() and (trace == 7).all() and (best == 7).all() and (cur == 7).all() and (count == 7).all()
    with pytest.raises(ValueError):
        hip.plane_select_polled(keys, errs, 12, 13)
    with pytest.raises(ValueError):
        hip.plane_select_polled(keys, errs[:4].contiguous(), 12, 4)


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def tilted():
    return QO.tilted_road_scenes()


def test_distil_rows_for_the_location_end_to_end(tilted, tmp_path):
    """ 96 Cars on 12 tilted roads, a random pool of 400 planes without the true ones.  Re-derived on the CPU with pair_costs_np and
    select_polled_np before any GPU run: all 96 objects served, the run stops after 40 picks (the key greedy after 48), the first eight
    picks differ between the two rules, the first pick's objective is 630 248 against 764 253 for the key greedy's first pick, the mean
    (median) polled location error is 1.18 m (0.70 m) against 1.80 m (0.91 m).  Asserted are the conditions, not those digits. """
    scenes, pool = tilted
    labels_list, P_list = [g for _, g, _ in scenes], [P for _, _, P in scenes]
    _, det = L.prepare_batch(np.stack(labels_list), [8] * 12, np.stack(P_list), det_types=L.CAR)
    served = (det[4] >= 0).reshape(-1)
    objects = int(served.sum())
    keys_d, errs_d, M = plane_db.cost_table(labels_list, P_list, pool, errors=True)
    keys, errs = u16(keys_d), u16(errs_d)
    assert M == 400 and keys.shape == (objects, 400) and errs.shape == (objects, 400)
    pinv = np.stack([np.linalg.pinv(P) for P in P_list]).astype(np.float32)
    want = np.stack(labels_list)[..., 11:14].astype(np.float32)
    host_k, host_e = plane_db.pair_costs_np(det[0], det[1], det[4], pinv, want, pool)
    assert np.array_equal(keys, host_k[served]) and np.array_equal(errs, host_e[served])

    whole = plane_db.distil_rows(labels_list, P_list, pool, 400, objective='location', report=True)
    count = whole['count']
    assert whole['objects'] == objects and whole['served'] == objects and 1 <= count < 400 and whole['objective'] == 'location'
    padded = np.concatenate([whole['indices'], -np.ones(400 - count, np.int32)])
    QO.check_result(keys, errs, 400, padded, whole['trace'], whole['best'], whole['cur'], count)
    assert whole['planes'].dtype == pool.dtype and np.array_equal(whole['planes'], pool[whole['indices']])
    assert whole['mean_location_m'] == whole['cur'].astype(np.int64).mean() / 256.0 == int(whole['trace'][-1]) / 256.0 / objects
    assert sorted(whole['prefixes']) == [n for n in (1, 10, 100) if n < count] and 'median_location_m' in whole['prefixes'][1]
    single = [int(plane_db.polled_state_np(keys, errs, [p])[1].astype(np.int64).sum()) for p in range(400)]
    assert int(whole['trace'][1]) == min(single) and whole['indices'][0] == single.index(min(single))
    # the two chunkings and the host selection give the same run
    chunked = plane_db.distil_rows(labels_list, P_list, pool, 400, objective='location', chunk_images=5)
    host = plane_db.distil_rows(labels_list, P_list, pool, 400, objective='location', device=False)
    for other in (chunked, host):
        for name in ('indices', 'trace', 'best', 'cur'):
            assert np.array_equal(other[name], whole[name]), name
    ten = plane_db.distil_rows(labels_list, P_list, pool, 10, objective='location')
    n = min(10, count)
    assert ten['count'] == n and np.array_equal(ten['indices'], whole['indices'][:n]) and np.array_equal(ten['trace'][:n + 1], whole['trace'][:n + 1])
    # the default objective picks other planes, and loses more location under this measure
    by_key = plane_db.distil_rows(labels_list, P_list, pool, 400)
    assert 'cur' not in by_key and by_key['indices'].tolist() != whole['indices'].tolist()
    _, cur_key = plane_db.polled_state_np(keys, errs, by_key['indices'])
    print('location: {} picks, {}; poll: {} picks, {}'.format(count, plane_db.location_summary(whole['cur']), by_key['count'], plane_db.location_summary(cur_key)))
    assert int(whole['trace'][1]) <= int(plane_db.polled_state_np(keys, errs, by_key['indices'][:1])[1].astype(np.int64).sum())

    # written, re-read, polled: polling serves every object with the plane the replay says, at the error the selection counted
    path = os.path.join(str(tmp_path), 'distilled.mat')
    plane_db.write_database(path, whole['planes'])
    planes = L._load_planes(path)
    assert np.array_equal(planes, whole['planes'].astype(np.float32))
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    _, _, residuals, index = gpp_utils.fit_road_planes(up(det[0]), up(det[1]), up(det[4]), up(pinv), up(planes), return_index=True)
    residuals, index = residuals.cpu().numpy().reshape(-1)[served], index.cpu().numpy().reshape(-1)[served]
    sub_k = keys[:, whole['indices']].astype(np.int64)       # the chosen planes in file order
    lowest = sub_k.min(axis=1)
    holder = sub_k.argmin(axis=1)                            # the first plane of the file that holds the smallest key: the replayed plane
    alone = (sub_k == lowest[:, None]).sum(axis=1) == 1
    checked = alone & (residuals < 16.0) & (lowest < 65535)
    print('objects checked against polling: {} of {}'.format(int(checked.sum()), objects))
    assert checked.sum() >= 0.9 * objects
    assert np.array_equal(index[checked], holder[checked])
    replayed = errs[np.arange(objects), whole['indices'][holder]]
    assert np.array_equal(replayed[lowest < 65535], whole['cur'][lowest < 65535])


def test_distil_planes_command_line_with_the_location_objective(tilted, tmp_path, capsys):
    import scipy.io
    scenes, pool = tilted
    label_dir, calib_dir = LO.write_dataset(tmp_path, scenes)
    pool_path, out = os.path.join(str(tmp_path), 'pool.mat'), os.path.join(str(tmp_path), 'out.mat')
    plane_db.write_database(pool_path, pool)
    result = distil_planes.main([label_dir, calib_dir, pool_path, out, '--objective', 'location', '--planes', '30', '--report'])
    lines = capsys.readouterr().out.splitlines()
    sizes = plane_db.prefix_sizes(result['count'])
    assert len(lines) == len(sizes) + 1 and all('location error mean' in line and ' m ' in line for line in lines[:-1])
    assert [int(line.split()[0]) for line in lines[:-1]] == sizes
    written = scipy.io.loadmat(out)['road_planes_database']
    assert written.shape == (result['count'], 4) and np.array_equal(written, pool[result['indices']])
    # the default objective's output is the one of a call without the option
    plain = distil_planes.main([label_dir, calib_dir, pool_path, out, '--planes', '30', '--report'])
    first = capsys.readouterr().out
    named = distil_planes.main([label_dir, calib_dir, pool_path, out, '--objective', 'poll', '--planes', '30', '--report'])
    assert capsys.readouterr().out == first and 'six votes' in first and np.array_equal(named['indices'], plain['indices'])
    assert plain['indices'].tolist() != result['indices'].tolist()
