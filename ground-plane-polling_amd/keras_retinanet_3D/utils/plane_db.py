"""
Distil a plane database: from a pool of candidate planes (the 22k file, or per-frame road fits of one's own) and a labelled dataset, the K
planes that ground-plane polling on that dataset loses least with -- DESIGN.md section 4.21 is the specification.  The reference ships
five fixed databases and tells the user to "replace road_planes_database.mat with relevant files of your own"; this module makes one.

    cost_table     labels -> keypoints (gpp_label_prep_f64) -> the (object, plane) table of 16-bit keys (gpp_poll_costs_u16, csrc/plane_db.hip)
    select         greedy facility location on the table on the device (gpp_plane_select)
    select_np      the same in NumPy integers: equal to the kernel entry for entry
    distil         label_2 + calib directories and a pool -> the chosen rows of the pool in pick order, with the objective's trace
    write_database the rows as a .mat that the rest of the project (and the reference) reads

The key of a pair: 65535 if the plane puts the object behind the camera or its residual is not finite, else
(6 - votes) * 8192 + min(floor(1024 * residual sum in metres), 8191) -- the order in which polling itself ranks planes.  The objective is
the sum over the objects of the best key among the chosen planes; every pick takes the plane that lowers it most (the first such plane),
so the picks of a run are a prefix of the picks of every longer run.

The device entry points raise GppError without a GPU, like polling_ceiling; select_np needs nothing but NumPy.
"""
import os

import numpy as np

from . import kitti_eval
from .label_prep import CAR, _check_alpha, _load_planes, _upload, read_calibration

INVALID = 65535                                             # GPP_PLANE_COST_INVALID (include/gpp.h)
VOTE_STEP = 8192                                            # key = (6 - votes) * VOTE_STEP + residual quantum
QUANTA_PER_M = 1024.0
DATABASE_KEY = 'road_planes_database'


# ---------------------------------------------------------------------------------------------------- the host form of the selection
def select_np(table, k):
    """ greedy facility location on table (O, M) of uint16 keys, k picks, in NumPy integers: the host form of gpp_plane_select.
    Returns {'chosen' (k,) int32, 'trace' (k + 1,) uint64, 'best' (O,) uint16, 'count' int}: pick j takes the FIRST plane of the largest
    gain sum_o max(0, best[o] - table[o][p]); a largest gain of 0 ends the run (chosen -1 from there on, the trace repeats). """
    table = np.asarray(table)
    if table.ndim != 2 or table.dtype != np.uint16:
        raise ValueError('table must be (O, M) uint16, got {} {}'.format(table.shape, table.dtype))
    O, M = table.shape
    k = int(k)
    if O < 1 or M < 1 or k < 1 or k > M:
        raise ValueError('O = {}, M = {}, k = {}: needs O >= 1 and 1 <= k <= M'.format(O, M, k))
    t = table.astype(np.int32)
    best = np.full(O, INVALID, np.int32)
    chosen = np.full(k, -1, np.int32)
    trace = np.empty(k + 1, np.uint64)
    trace[0] = INVALID * O
    count = 0
    for j in range(k):
        gain = np.maximum(best[:, None] - t, 0).sum(axis=0, dtype=np.int64)
        p = int(np.argmax(gain))                             # the first maximum
        if gain[p] == 0:
            break
        chosen[j], count = p, j + 1
        best = np.minimum(best, t[:, p])
        trace[j + 1] = int(trace[j]) - int(gain[p])
    trace[count + 1:] = trace[count]
    return {'chosen': chosen, 'trace': trace, 'best': best.astype(np.uint16), 'count': count}


def objective(table, chosen):
    """ sum over the rows of the smallest key among the columns `chosen` (65535 per row when there are none): what trace[len(chosen)] holds """
    table = np.asarray(table)
    chosen = [int(p) for p in chosen if int(p) >= 0]
    if not chosen:
        return INVALID * table.shape[0]
    return int(table[:, chosen].min(axis=1).astype(np.int64).sum())


def best_summary(best):
    """ what `best` (O,) uint16 says about the chosen planes: the share of objects whose best plane has all six votes, and the median over
    the objects some plane serves of that plane's residual in metres per segment (the quantised residual sum / 6, as gpp_poll_f32
    reports residuals; the quantum saturates at 8191 / 1024 m) """
    best = np.asarray(best).astype(np.int64)
    served = best[best < INVALID]
    return {'objects': int(best.size), 'served': int(served.size),
            'six_vote_share': float((best < VOTE_STEP).sum()) / best.size if best.size else 0.0,
            'median_residual_m': float(np.median((served % VOTE_STEP) / QUANTA_PER_M / 6.0)) if served.size else float('nan')}


# ---------------------------------------------------------------------------------------------------- the device side
def cost_table(labels_list, P_list, pool, det_types=CAR, thr=0.7, chunk_images=None):
    """ the cost table of a dataset on the device: per image the (n, 16) labels and the (3, 4) matrix, pool (M, 4) -> (table, M) with
    table an (O, pitch) int16 device tensor of uint16 keys, one row per label that is a detection of `det_types` (in image, then label
    order), pitch = M rounded up to 8, the pad columns 65535.  Chunked as polling_ceiling is: per chunk labels, trig, P and pinv(P) go up
    once, gpp_label_prep_f64 (own_box) fills the decode layout, the rows with orient >= 0 are listed on the device and
    gpp_poll_costs_u16 fills its rows.  Raises GppError without a GPU, MemoryError when the table does not fit the free device memory. """
    import torch
    from ..backend import hip
    dev = hip.require_device()
    if len(labels_list) != len(P_list):
        raise ValueError('{} label arrays and {} matrices'.format(len(labels_list), len(P_list)))
    pool32 = _load_planes(pool)
    M = pool32.shape[0]
    planes_d = torch.as_tensor(pool32).to(dev)
    A = max([np.asarray(g).reshape(-1, kitti_eval.LABEL_COLS).shape[0] for g in labels_list] + [1])
    if A > kitti_eval.MAX_LABELS:
        raise ValueError('the device form takes up to {} labels per image, got {}'.format(kitti_eval.MAX_LABELS, A))
    step = kitti_eval.chunk_images(A, A) if chunk_images is None else max(1, int(chunk_images))
    parts = []
    for at in range(0, len(labels_list), step):
        part_labels, part_P = labels_list[at:at + step], P_list[at:at + step]
        labels_d, counts_d, P_d, trig_d = _upload(part_labels, part_P, A, dev)
        pinv = np.stack([np.linalg.pinv(np.asarray(P, np.float64).reshape(3, 4)) for P in part_P]).astype(np.float32)
        pinv_d = torch.as_tensor(pinv).to(dev, non_blocking=True)
        _, (boxes, dims, _, _, orient) = hip.label_prep(labels_d, counts_d, P_d, trig_d, det_types, True, True)
        rows = torch.nonzero(orient.reshape(-1) >= 0).reshape(-1).to(torch.int32)          # ascending: image, then label order
        parts.append((boxes, dims, orient, pinv_d, rows))
    O = sum(int(p[4].numel()) for p in parts)
    pitch = hip.table_pitch(M)
    free = torch.cuda.mem_get_info(dev)[0]
    if O * pitch * 2 > free:
        raise MemoryError('the cost table of {} objects x {} planes needs {:.2f} GB, {:.2f} GB of device memory are free: '
                          'use a smaller pool or fewer labels'.format(O, M, O * pitch * 2 / 1e9, free / 1e9))
    table = torch.full((O, pitch), -1, dtype=torch.int16, device=dev)                      # int16 -1 = the key 65535
    at = 0
    for boxes, dims, orient, pinv_d, rows in parts:
        if rows.numel():
            at += hip.poll_costs(boxes, dims, orient, pinv_d, planes_d, table, rows, at, thr)
    return table, M


def select(table, M, k):
    """ gpp_plane_select on a device table -> the dict of select_np (NumPy, fetched once at the end) """
    import torch
    from ..backend import hip
    chosen, trace, best, count = hip.plane_select(table, M, k)
    torch.cuda.synchronize(table.device)
    return {'chosen': chosen.cpu().numpy(), 'trace': trace.cpu().numpy().view(np.uint64), 'best': best.cpu().numpy().view(np.uint16),
            'count': int(count.item())}


def _result(pool, picked, objects):
    count = picked['count']
    indices = picked['chosen'][:count].copy()
    return dict(best_summary(picked['best']), planes=np.ascontiguousarray(np.asarray(pool).reshape(-1, 4)[indices]), indices=indices,
                trace=picked['trace'], count=count, objects=objects, best=picked['best'])


def distil_rows(labels_list, P_list, pool, k, device=True, det_types=CAR, thr=0.7, chunk_images=None, report=False):
    """ distil on arrays already in memory: per image the (n, 16) labels (kitti_eval.read_label_file) and the (3, 4) camera matrix, pool
    (M, 4) or the path of a .mat -> dict
        planes   (count, 4)  the chosen rows of the pool, verbatim, in pick order, in the pool's own dtype (not canonicalised)
        indices  (count,)    their rows in the pool;  count <= k: the run ends when no plane lowers the objective
        trace    (k + 1,)    uint64, the objective after 0 .. k picks: every prefix of `planes` is the distillation of its length
        objects, served, six_vote_share, median_residual_m, best: best_summary of the final state
        prefixes (with `report`): {n: best_summary} of the prefixes of 1, 10, 100 ... planes -- each a shorter run of the selection
    The cost table is always made on the device; device=False runs the selection in NumPy (select_np) instead of gpp_plane_select. """
    if isinstance(pool, (str, bytes, os.PathLike)):
        import scipy.io
        pool = scipy.io.loadmat(pool)[DATABASE_KEY]
    pool = np.asarray(pool)
    if pool.ndim != 2 or pool.shape[1] != 4 or pool.shape[0] < 1:
        raise ValueError('the pool must be (M, 4) with M >= 1, got {}'.format(pool.shape))
    k = int(k)
    if k < 1 or k > pool.shape[0]:
        raise ValueError('{} planes asked of a pool of {}'.format(k, pool.shape[0]))
    table, M = cost_table(labels_list, P_list, pool, det_types, thr, chunk_images)
    O = int(table.shape[0])
    if O < 1:
        raise ValueError('the dataset has no object of the asked types in front of the camera')
    host = None if device else table[:, :M].cpu().numpy().view(np.uint16)
    run = (lambda n: select(table, M, n)) if device else (lambda n: select_np(host, n))
    picked = run(k)
    result = _result(pool, picked, O)
    if report:
        result['prefixes'] = {}
        for n in prefix_sizes(picked['count'])[:-1]:
            short = run(n)
            if not np.array_equal(short['chosen'], picked['chosen'][:n]):
                raise RuntimeError('the run of {} picks is no prefix of the run of {}'.format(n, k))
            result['prefixes'][n] = best_summary(short['best'])
    return result


def distil(label_dir, calib_dir, pool, k, device=True, det_types=CAR, thr=0.7, report=False):
    """ distil_rows on the label_2 files of `label_dir` (sorted by name) and the calibration files of the same names in `calib_dir` """
    files = sorted(f for f in os.listdir(label_dir) if f.endswith('.txt'))
    labels_list = [kitti_eval.read_label_file(os.path.join(label_dir, f)) for f in files]
    P_list = [read_calibration(os.path.join(calib_dir, f)) for f in files]
    for f, g, P in zip(files, labels_list, P_list):
        try:
            _check_alpha(g, P)
        except ValueError as e:
            raise ValueError('{}: {}'.format(os.path.join(label_dir, f), e))
    return distil_rows(labels_list, P_list, pool, k, device, det_types, thr, report=report)


# ---------------------------------------------------------------------------------------------------- files
def write_database(path, planes):
    """ planes (N, 4) -> a .mat under the key road_planes_database, as the shipped databases are stored (utils.label_prep._load_planes,
    utils.synthetic.load_plane_database and the reference's run_network.py read it back) """
    import scipy.io
    planes = np.asarray(planes)
    if planes.ndim != 2 or planes.shape[1] != 4 or planes.shape[0] < 1:
        raise ValueError('planes must be (N, 4) with N >= 1, got {}'.format(planes.shape))
    scipy.io.savemat(path, {DATABASE_KEY: planes})


def prefix_sizes(count):
    """ 1, 10, 100 ... below `count`, then `count` itself """
    return sorted({10 ** e for e in range(0, 10) if 10 ** e < count} | ({count} if count > 0 else set()))


def prefix_report(result):
    """ one line per power of ten of the prefix and one for the whole run: planes, the objective and, where known (the whole run; the
    prefixes of a run made with `report`), the six-vote share and the median residual """
    lines = []
    for n in prefix_sizes(result['count']):
        s = result if n == result['count'] else result.get('prefixes', {}).get(n)
        share = '   six votes {:7.2%}   median residual {:.4f} m'.format(s['six_vote_share'], s['median_residual_m']) if s else ''
        lines.append('{:8d} planes   objective {:16d}   per object {:10.2f}{}'.format(
            n, int(result['trace'][n]), int(result['trace'][n]) / max(1, result['objects']), share))
    return lines
