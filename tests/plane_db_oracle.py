""" ORACLE (test infrastructure): the plane distillation written as plain loops, and the cost table composed from the
functions of oracle/polling_np.py with the key formula of include/gpp.h.  Shared by tests/test_plane_db_cpu.py and _gpu.py. """
import numpy as np

INVALID = 65535


def select_loops(table, k):
    """ greedy facility location with Python integers and explicit loops: (chosen list of k, trace list of k + 1, best list, count) """
    rows = [[int(v) for v in r] for r in np.asarray(table)]
    O, M = len(rows), len(rows[0])
    best = [INVALID] * O
    chosen, trace, count = [-1] * k, [INVALID * O] * (k + 1), 0
    for j in range(k):
        top, at = 0, -1
        for p in range(M):
            gain = 0
            for o in range(O):
                if best[o] > rows[o][p]:
                    gain += best[o] - rows[o][p]
            if gain > top:                                  # strictly greater: the first index of the largest gain stays
                top, at = gain, p
        if at < 0:
            break
        chosen[j], count = at, j + 1
        for o in range(O):
            best[o] = min(best[o], rows[o][at])
        trace[j + 1] = trace[j] - top
    for j in range(count + 1, k + 1):
        trace[j] = trace[count]
    return chosen, trace, best, count


def seeded_table(seed, O, M, special=True):
    """ (O, M) uint16 keys as gpp_poll_costs_u16 makes them: (6 - votes) * 8192 + q or 65535, with 0, 57343 and 65535 present """
    rng = np.random.default_rng(seed)
    t = (rng.integers(0, 7, size=(O, M)) * 8192 + rng.integers(0, 8192, size=(O, M))).astype(np.int64)
    t[rng.random((O, M)) < 0.2] = INVALID
    if special:
        flat = t.reshape(-1)
        for v in (0, 57343, INVALID):
            flat[rng.integers(0, flat.size)] = v
    return t.astype(np.uint16)


def check_result(table, k, chosen, trace, best, count):
    """ the properties every run has, whoever computed it """
    table = np.asarray(table).astype(np.int64)
    O = table.shape[0]
    chosen, trace, best = [int(v) for v in chosen], [int(v) for v in trace], [int(v) for v in best]
    assert len(chosen) == k and len(trace) == k + 1 and len(best) == O and 0 <= count <= k
    assert trace[0] == INVALID * O
    assert all(p >= 0 for p in chosen[:count]) and all(p == -1 for p in chosen[count:])
    assert len(set(chosen[:count])) == count                                              # never the same plane twice
    assert all(trace[j + 1] < trace[j] for j in range(count))                             # strictly down to count
    assert all(trace[j] == trace[count] for j in range(count, k + 1))                     # constant from there
    for j in range(count + 1):                                                            # recomputed from the picks
        want = table[:, chosen[:j]].min(axis=1).sum() if j else INVALID * O
        assert trace[j] == want, j
    want_best = table[:, chosen[:count]].min(axis=1) if count else np.full(O, INVALID)
    assert best == want_best.tolist()


def cost_keys(boxes, dims, orient, P_inv, planes, thr=0.7):
    """ the table of gpp_poll_costs_u16 for every row of the batch, (B * D, M) uint16: canonical_planes, back_project, hypotheses,
    poll_targets and poll of oracle/polling_np.py, then the key formula in float32 """
    from oracle import polling_np as PN
    F = np.float32
    assert F(thr) == PN.POLL_THRESHOLD
    B, D = np.asarray(orient).shape
    planes_c = np.tile(PN.canonical_planes(planes)[None], (B, 1, 1))
    with np.errstate(all='ignore'):
        rays = PN.back_project(boxes, P_inv)
        X, zc = PN.hypotheses(rays, planes_c)
        targets = PN.poll_targets(dims, orient)
        votes = res = None
        for (a, b), t in zip(PN.POLL_SEGMENTS, targets):
            v, r = PN.poll(X[..., a, :], X[..., b, :], t[..., None])
            votes = v if votes is None else votes + v
            res = r if res is None else res + r
        assert votes.dtype == F and res.dtype == F and zc.dtype == F
        invalid = (zc < F(0.0)) | ~(res < np.finfo(F).max)
        s = res * F(1024.0)
        q = np.where(s < F(8191.0), np.where(invalid, F(0.0), s).astype(np.int64), 8191)
        key = (6 - votes.astype(np.int64)) * 8192 + q
    key = np.where(invalid, INVALID, key)
    key = np.where((np.asarray(orient) < 0)[..., None], INVALID, key)
    return key.reshape(B * D, -1).astype(np.uint16), votes.reshape(B * D, -1), res.reshape(B * D, -1), zc.reshape(B * D, -1)
