""" The loop-written oracle of the offline smoother (include/gpp.h, gpp_track_smooth_f64): segments, the forward
filter of section 4.34, the backward Rauch-Tung-Striebel pass and the outputs, one segment, one cell and one Python float operation at a
time.  Python floats are IEEE doubles and nothing here is fused, so every word equals the NumPy form's (utils/track_smooth.py) and the
kernel's; atan2 alone (column 25) is the platform's.  2 x 2 blocks are nested lists [[xx, xz], [zx, zz]]. """
import math

import numpy as np

PI = math.pi
TWO_PI = 2.0 * math.pi
CODE_COLS = (13, 14, 33, 34, 35)


def wrap(a):
    a = a - TWO_PI * math.floor(a / TWO_PI)
    if a < 0.0:
        a += TWO_PI
    if a >= TWO_PI:
        a -= TWO_PI
    if a >= PI:
        a -= TWO_PI
    return a


def div(a, b):
    """ IEEE division: Python raises where the rule has an infinity or a NaN """
    return float(np.float64(a) / np.float64(b))


def times(a, b):
    return float(np.float64(a) * np.float64(b))                          # (an overflow is an infinity, not an OverflowError)


def mul(X, Y):
    return [[times(X[i][0], Y[0][j]) + times(X[i][1], Y[1][j]) for j in range(2)] for i in range(2)]


def tr(X):
    return [[X[0][0], X[1][0]], [X[0][1], X[1][1]]]


def add(X, Y):
    return [[X[i][j] + Y[i][j] for j in range(2)] for i in range(2)]


def sub(X, Y):
    return [[X[i][j] - Y[i][j] for j in range(2)] for i in range(2)]


def sym(xx, xz, zz):
    return [[xx, xz], [xz, zz]]


def segments(ids, seq_start, max_gap, rows=None):
    """ -> a list of (id, first frame, [row index or -1 per cell]) ordered by (sequence, id, first frame); ValueError for an id twice in a frame """
    N, D = len(ids), (len(ids[0]) if len(ids) else 0)
    seq_start = [0, N] if seq_start is None else list(seq_start)
    out = []
    for s in range(len(seq_start) - 1):
        seen = {}
        for f in range(seq_start[s], seq_start[s + 1]):
            here = set()
            for d in range(D):
                who = int(ids[f][d])
                if who < 0 or (rows is not None and (math.isnan(rows[f][d][19]) or math.isnan(rows[f][d][21]))):
                    continue
                if who in here:
                    raise ValueError('the id {} stands twice in frame {}'.format(who, f))
                here.add(who)
                seen.setdefault(who, []).append((f, f * D + d))
        for who in sorted(seen):
            run = []
            for f, r in seen[who]:
                if run and f - run[-1][0] > max_gap + 1:
                    out.append(close(who, run))
                    run = []
                run.append((f, r))
            out.append(close(who, run))
    return out


def close(who, run):
    cells = [-1] * (run[-1][0] - run[0][0] + 1)
    for f, r in run:
        cells[f - run[0][0]] = r
    return who, run[0][0], cells


def row_noise(x, z, noise):
    (r0, r1), (t0, t1) = noise['radial'], noise['tangential']
    rho = math.sqrt(times(x, x) + times(z, z))
    ux, uz = (div(x, rho), div(z, rho)) if rho != 0.0 else (0.0, 1.0)
    sr, st = r0 + times(r1, rho), t0 + times(t1, rho)
    vr, vt = times(sr, sr), times(st, st)
    dv = vr - vt
    return sym(vt + times(dv, times(ux, ux)), times(dv, times(ux, uz)), vt + times(dv, times(uz, uz)))


def born(x, z, R, speed):
    return {'p': [x, z], 'v': [0.0, 0.0], 'A': [list(R[0]), list(R[1])], 'B': [[0.0, 0.0], [0.0, 0.0]], 'C': sym(speed * speed, 0.0, speed * speed)}


def predict(s, q_pos, q_vel):
    A, B, C = s['A'], s['B'], s['C']
    return {'p': [s['p'][0] + s['v'][0], s['p'][1] + s['v'][1]], 'v': list(s['v']),
            'A': sym(((A[0][0] + (B[0][0] + B[0][0])) + C[0][0]) + q_pos, (A[0][1] + (B[0][1] + B[1][0])) + C[0][1],
                     ((A[1][1] + (B[1][1] + B[1][1])) + C[1][1]) + q_pos),
            'B': [[B[0][0] + C[0][0], B[0][1] + C[0][1]], [B[1][0] + C[0][1], B[1][1] + C[1][1]]],
            'C': sym(C[0][0] + q_vel, C[0][1], C[1][1] + q_vel)}


def ego_step(s, g, t0, t2):
    gt = tr(g)
    A, C = mul(mul(g, s['A']), gt), mul(mul(g, s['C']), gt)
    return {'p': [(times(g[0][0], s['p'][0]) + times(g[0][1], s['p'][1])) + t0, (times(g[1][0], s['p'][0]) + times(g[1][1], s['p'][1])) + t2],
            'v': [times(g[0][0], s['v'][0]) + times(g[0][1], s['v'][1]), times(g[1][0], s['v'][0]) + times(g[1][1], s['v'][1])],
            'A': sym(A[0][0], A[0][1], A[1][1]), 'B': mul(mul(g, s['B']), gt), 'C': sym(C[0][0], C[0][1], C[1][1])}


def update(s, xr, zr, R):
    """ -> the updated state, or None when det is not > 0 """
    A, B, C = s['A'], s['B'], s['C']
    S = add(A, R)
    det = times(S[0][0], S[1][1]) - times(S[0][1], S[0][1])
    if not det > 0.0:
        return None
    d = [xr - s['p'][0], zr - s['p'][1]]
    iS = sym(div(S[1][1], det), -div(S[0][1], det), div(S[0][0], det))
    K = mul(sym(A[0][0], A[0][1], A[1][1]), iS)                          # rows x, z
    Lg = mul(tr(B), iS)                                                  # rows vx, vz
    KA, KB, LB = mul(K, sym(A[0][0], A[0][1], A[1][1])), mul(K, B), mul(Lg, B)
    return {'p': [s['p'][i] + (times(K[i][0], d[0]) + times(K[i][1], d[1])) for i in range(2)],
            'v': [s['v'][i] + (times(Lg[i][0], d[0]) + times(Lg[i][1], d[1])) for i in range(2)],
            'A': sym(A[0][0] - KA[0][0], A[0][1] - KA[0][1], A[1][1] - KA[1][1]), 'B': sub(B, KB),
            'C': sym(C[0][0] - LB[0][0], C[0][1] - LB[0][1], C[1][1] - LB[1][1])}


def back(sm, pp, pf, g):
    """ one backward step -> the smoothed state of cell c, or None when a determinant is not > 0 (the step is skipped) """
    A, B, C = pp['A'], pp['B'], pp['C']
    dA = times(A[0][0], A[1][1]) - times(A[0][1], A[0][1])
    if not dA > 0.0:
        return None
    iA = sym(div(A[1][1], dA), -div(A[0][1], dA), div(A[0][0], dA))
    W = mul(iA, B)
    Tm = mul(tr(B), W)
    sxx, sxz, szz = C[0][0] - Tm[0][0], C[0][1] - Tm[0][1], C[1][1] - Tm[1][1]
    dS = times(sxx, szz) - times(sxz, sxz)
    if not dS > 0.0:
        return None
    iS = sym(div(szz, dS), -div(sxz, dS), div(sxx, dS))
    Fm = [[-v for v in line] for line in mul(W, iS)]
    E = sub(iA, mul(Fm, tr(W)))
    U = [[add(pf['A'], pf['B']), pf['B']], [add(tr(pf['B']), pf['C']), pf['C']]]
    if g is not None:
        U = [[mul(block, tr(g)) for block in line] for line in U]
    inverse = [[E, Fm], [tr(Fm), iS]]
    J = [[add(mul(U[i][0], inverse[0][j]), mul(U[i][1], inverse[1][j])) for j in range(2)] for i in range(2)]
    dp = [sm['p'][0] - pp['p'][0], sm['p'][1] - pp['p'][1]]
    dv = [sm['v'][0] - pp['v'][0], sm['v'][1] - pp['v'][1]]
    Dm = [[sub(sm['A'], A), sub(sm['B'], B)], [tr(sub(sm['B'], B)), sub(sm['C'], C)]]
    Nm = [[add(mul(J[i][0], Dm[0][j]), mul(J[i][1], Dm[1][j])) for j in range(2)] for i in range(2)]
    QA = add(mul(Nm[0][0], tr(J[0][0])), mul(Nm[0][1], tr(J[0][1])))
    QB = add(mul(Nm[0][0], tr(J[1][0])), mul(Nm[0][1], tr(J[1][1])))
    QC = add(mul(Nm[1][0], tr(J[1][0])), mul(Nm[1][1], tr(J[1][1])))
    mean = [[pf[name][i] + ((times(J[h][0][i][0], dp[0]) + times(J[h][0][i][1], dp[1])) + (times(J[h][1][i][0], dv[0]) + times(J[h][1][i][1], dv[1])))
             for i in range(2)] for h, name in enumerate(('p', 'v'))]
    return {'p': mean[0], 'v': mean[1], 'A': sym(pf['A'][0][0] + QA[0][0], pf['A'][0][1] + QA[0][1], pf['A'][1][1] + QA[1][1]),
            'B': add(pf['B'], QB), 'C': sym(pf['C'][0][0] + QC[0][0], pf['C'][0][1] + QC[0][1], pf['C'][1][1] + QC[1][1])}


def words(s):
    """ a state as the 14 words x z vx vz Axx Axz Azz Bxx Bxz Bzx Bzz Cxx Cxz Czz """
    return s['p'] + s['v'] + [s['A'][0][0], s['A'][0][1], s['A'][1][1], s['B'][0][0], s['B'][0][1], s['B'][1][0], s['B'][1][1],
                              s['C'][0][0], s['C'][0][1], s['C'][1][1]]


def smooth_segment(flat, cells, frame, noise, ego):
    """ one segment of two or more cells -> per cell (predicted or None, filtered, smoothed) """
    q_pos, q_vel = noise['process']
    speed = noise['birth_speed']
    x, z = float(flat[cells[0]][19]), float(flat[cells[0]][21])
    cur = born(x, z, row_noise(x, z, noise), speed)
    pred, filt, restart = [None], [cur], [False]
    for c in range(1, len(cells)):
        cur = predict(cur, q_pos, q_vel)
        if ego is not None:
            e = [float(v) for v in ego[frame + c]]
            cur = ego_step(cur, [[e[0], e[2]], [e[6], e[8]]], e[9], e[11])
        pred.append(cur)
        again = False
        if cells[c] >= 0:
            x, z = float(flat[cells[c]][19]), float(flat[cells[c]][21])
            R = row_noise(x, z, noise)
            new = update(cur, x, z, R)
            again = new is None
            cur = born(x, z, R, speed) if again else new
        restart.append(again)
        filt.append(cur)
    sm = [None] * len(cells)
    sm[-1] = filt[-1]
    for c in range(len(cells) - 2, -1, -1):
        g = None
        if ego is not None:
            e = [float(v) for v in ego[frame + c + 1]]
            g = [[e[0], e[2]], [e[6], e[8]]]
        new = None if restart[c + 1] else back(sm[c + 1], pred[c + 1], filt[c], g)
        sm[c] = filt[c] if new is None else new
    return pred, filt, sm


def smooth(rows, segs, noise, ego=None, keep=None):
    """ rows (N, D, 36) float32, segs: segments()' list (in any order) -> (rows_out, row_cov (N, D, 3), fill_rows (fills, 36), fill_cov
    (fills, 3)); keep: a list that receives per segment (predicted, filtered, smoothed), each a list of 14 words per cell (None: none) """
    rows = np.asarray(rows, np.float32)
    N, D = rows.shape[:2]
    flat = rows.reshape(-1, 36)
    out = flat.copy()
    row_cov = np.zeros((N * D, 3))
    fills, fill_cov = [], []
    with np.errstate(all='ignore'):
        for who, frame, cells in segs:
            if len(cells) < 2:
                if keep is not None:
                    keep.append(None)
                continue
            pred, filt, sm = smooth_segment(flat, cells, frame, noise, ego)
            if keep is not None:
                keep.append(([None if p is None else words(p) for p in pred], [words(s) for s in filt], [words(s) for s in sm]))
            for c, r in enumerate(cells):
                xs, zs = sm[c]['p']
                cov = [sm[c]['A'][0][0], sm[c]['A'][0][1], sm[c]['A'][1][1]]
                if r >= 0:
                    out[r, 19], out[r, 21] = np.float32(xs), np.float32(zs)
                    out[r, 25] = np.float32(wrap(float(flat[r][32]) - math.atan2(xs, zs)))
                    row_cov[r] = cov
                    continue
                c0 = max(k for k in range(c) if cells[k] >= 0)
                c1 = min(k for k in range(c + 1, len(cells)) if cells[k] >= 0)
                a, b = flat[cells[c0]], flat[cells[c1]]
                w = float(c - c0) / float(c1 - c0)
                fill = np.zeros(36, np.float32)
                for col in range(36):
                    fill[col] = a[col] if col in CODE_COLS else np.float32(float(a[col]) + times(w, float(b[col]) - float(a[col])))
                delta = wrap(float(b[32]) - float(a[32]))
                if delta >= PI / 2.0:
                    delta -= PI
                if delta < -(PI / 2.0):
                    delta += PI
                ry = wrap(float(a[32]) + w * delta)
                fill[19], fill[21], fill[32] = np.float32(xs), np.float32(zs), np.float32(ry)
                fill[25] = np.float32(wrap(ry - math.atan2(xs, zs)))
                fills.append(fill)
                fill_cov.append(cov)
    return (out.reshape(N, D, 36), row_cov.reshape(N, D, 3), np.array(fills, np.float32).reshape(-1, 36), np.array(fill_cov, np.float64).reshape(-1, 3))
