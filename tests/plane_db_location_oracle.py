""" ORACLE (test infrastructure): the selection for the polled location error written as plain loops over Python
integers, seeded paired tables, the properties every run has, and the inputs of the cost-table tests.  Shared by
tests/test_plane_db_location_cpu.py and _gpu.py. """
import numpy as np

INVALID = 65535
M_MAX = 1031
PAD_ROW, NAN_ROW = (1, 4), (0, 2)


def select_polled_loops(keys, errs, k):
    """ (chosen list of k, trace list of k + 1, best list, cur list, count), with Python integers and explicit loops """
    kr = [[int(v) for v in r] for r in np.asarray(keys)]
    er = [[int(v) for v in r] for r in np.asarray(errs)]
    O, M = len(kr), len(kr[0])
    best, cur = [INVALID] * O, [INVALID] * O
    chosen, trace, count = [-1] * k, [INVALID * O] * (k + 1), 0
    for j in range(k):
        top, at = 0, -1
        for p in range(M):
            gain = 0
            for o in range(O):
                if kr[o][p] < best[o]:
                    gain += cur[o] - er[o][p]                 # may be negative
            if gain > top:                                    # strictly greater: the first index of the largest gain stays
                top, at = gain, p
        if at < 0:                                            # the largest gain is at most 0
            break
        chosen[j], count = at, j + 1
        for o in range(O):
            if kr[o][at] < best[o]:
                best[o], cur[o] = kr[o][at], er[o][at]
        trace[j + 1] = trace[j] - top
    for j in range(count + 1, k + 1):
        trace[j] = trace[count]
    return chosen, trace, best, cur, count


def replay_loops(keys, errs, order):
    """ (best, cur) lists after the planes `order`, in that order: the first plane of the smallest key serves a row """
    keys, errs = np.asarray(keys), np.asarray(errs)
    O = keys.shape[0]
    best, cur = [INVALID] * O, [INVALID] * O
    for p in order:
        for o in range(O):
            if int(keys[o, p]) < best[o]:
                best[o], cur[o] = int(keys[o, p]), int(errs[o, p])
    return best, cur


def seeded_pair(seed, O, M, special=True):
    """ (keys, errs) (O, M) uint16 as gpp_pose_costs_u16 makes them: keys (6 - votes) * 8192 + q or 65535 (20 % of the pairs), errs drawn
    independently of the keys in [0, 65534], 65535 exactly where the key is; with `special` 0, 65534 and 65535 are present in errs (and 0,
    57343, 65535 in keys) whenever the table has room """
    rng = np.random.default_rng(seed)
    k = (rng.integers(0, 7, size=(O, M)) * 8192 + rng.integers(0, 8192, size=(O, M))).astype(np.int64)
    # location errors of every size: most within a few metres (small quanta), some far out
    e = np.where(rng.random((O, M)) < 0.7, rng.integers(0, 2048, size=(O, M)), rng.integers(0, 65535, size=(O, M))).astype(np.int64)
    k[rng.random((O, M)) < 0.2] = INVALID
    if special and O * M >= 8:
        cells = rng.permutation(O * M)[:5]
        for cell, (kv, ev) in zip(cells, ((0, 0), (57343, 65534), (INVALID, INVALID), (8192, 65534), (100, 0))):
            k.reshape(-1)[cell], e.reshape(-1)[cell] = kv, ev
    e[k == INVALID] = INVALID
    return k.astype(np.uint16), e.astype(np.uint16)


def check_result(keys, errs, k, chosen, trace, best, cur, count):
    """ the properties every run has, whoever computed it: the trace, best and cur recomputed by replaying the picks """
    O = np.asarray(keys).shape[0]
    chosen, trace = [int(v) for v in chosen], [int(v) for v in trace]
    best, cur = [int(v) for v in best], [int(v) for v in cur]
    assert len(chosen) == k and len(trace) == k + 1 and len(best) == O and len(cur) == O and 0 <= count <= k
    assert trace[0] == INVALID * O
    assert all(p >= 0 for p in chosen[:count]) and all(p == -1 for p in chosen[count:])
    assert len(set(chosen[:count])) == count                                              # never the same plane twice
    assert all(trace[j + 1] < trace[j] for j in range(count))                             # strictly down to count
    assert all(trace[j] == trace[count] for j in range(count, k + 1))                     # constant from there
    for j in range(count + 1):                                                            # trace[j] = the sum of cur after j picks
        b, c = replay_loops(keys, errs, chosen[:j])
        assert trace[j] == sum(c), j
    assert best == b and cur == c
    assert all((bb == INVALID) == (cc == INVALID) for bb, cc in zip(best, cur))


def polling_inputs(seed=11):
    """ the batch of tests/test_plane_db_gpu.polling_inputs, recreated: B = 2 images of D = 5 detections on rows of the pool; one -1
    padding row, one row whose top keypoint is NaN; the pool 600 rows of the shipped 22k database and seeded planes of every attitude
    (steep ones give zc < 0).  Added here: `want` (2, 5, 3) float32, per row the location that pool[0] (a plane of the road) gives it plus
    seeded noise of half a metre -- errors of centimetres to beyond the saturation, whichever plane is asked. """
    from keras_retinanet_3D.utils import plane_db, synthetic
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
    zero = np.zeros((2, 5, 3), np.float32)
    loc = plane_db.pair_costs_np(boxes, dims, orient, inp['P_inv'], zero, pool[:1], return_locations=True)[2].reshape(2, 5, 3)
    centre = np.where(np.isfinite(loc).all(axis=-1, keepdims=True), loc, np.array([0.0, 1.65, 20.0], np.float32))
    want = (centre + np.random.default_rng(seed + 1).normal(0.0, 0.5, size=(2, 5, 3))).astype(np.float32)
    return {'boxes': boxes, 'dims': dims, 'orient': orient, 'P_inv': inp['P_inv'], 'want': want, 'pool': pool}


# ---------------------------------------------------------------------------------------------------- the end-to-end scene of the issue
def tilted_road_scenes():
    """ 12 images of 8 Cars, each image on a tilted road of its own, the labels' height rounded to two decimals; a random pool of 400
    planes that holds none of the true ones.  -> (scenes [(names, labels, P)], pool (400, 4) float32) """
    import label_prep_oracle as LO
    rng = np.random.default_rng(4)
    scenes = []
    for b in range(12):
        labels, P = LO.seeded_scene(100 + b, 8, P_offset=False, kinds=(0,), behind=0.0)
        a = rng.normal(0.0, 0.02)
        c = rng.normal(0.0, 0.02)
        d = rng.uniform(1.4, 1.9)
        labels[:, 12] = np.round(d + a * labels[:, 11] + c * labels[:, 13], 2)
        scenes.append((['Car'] * 8, labels, P))
    pool = np.stack([rng.normal(0.0, 0.03, 400), -np.ones(400), rng.normal(0.0, 0.03, 400), rng.uniform(1.2, 2.1, 400)], axis=1).astype(np.float32)
    return scenes, pool
