""" Crowded scenes for the tracker (csrc/track.hip, DESIGN.md sections 4.28, 4.32 and 4.33) and a transcription of the kernel's greedy
phase 4.  The specification, the host form (utils/track.py: greedy) and the oracle (tests/track_oracle.py: step) state the association as
a serial rule; the kernel takes mutually-best pairs in rounds, keeps four 64-bit masks, gates the pairs in chunks of 4096 and clips the
survivors with all 128 lanes.  The scenes here are the ones in which those statements differ from the serial rule unless they are right:
many rounds, indices on both sides of 64, full and ragged chunks, matches on the chunks' edges, 8-vertex polygons in every lane.  NumPy
and Python only, no device:
tests/test_track_crowd_cpu.py asserts what the scenes reach, tests/test_track_crowd_gpu.py runs the kernel on them.

Every scene is (N, 128, 36) float32; a car's row index and its slot index differ (seeded permutations of the row order), so matched
pairs straddle 64 in both directions. """
import functools
import math

import numpy as np

import track_ego_oracle as E
import track_optimal_oracle as P
import track_oracle as O
from cuboid_nms_oracle import clip, corners
from keras_retinanet_3D.utils import track as T
from track_oracle import options, padding, row

D = 128
CHUNK = 4096                                  # track.hip's kChunk: the pairs gated per round of phase 3
GATE_SLACK = (1.0 + 1.0 / 32.0) ** 2          # track.hip's kGateSlack
MASK = (1 << 64) - 1

CHAIN_SIZES = (2, 63, 64, 65, 128)
LATTICE_SIZES = ((64, 64), (65, 64), (100, 90), (128, 128))
BOUNDARY_SIZES = (128, 127)
CHAIN_SEED, LATTICE_SEED, BOUNDARY_SEED = 7, 9, 13
CROWD_SEED = 3                                # chosen on the CPU: tests/test_track_crowd_cpu.py asserts the margins, every metric, both assignments
CROWD_GAINS = (0.6, 0.3, 0.1)


# ---------------------------------------------------------------------------------------------------- the scenes
def chain(n, seed=CHAIN_SEED):
    """ n slots and n rows alternate on a line at z = 20: slot 0, row 0, slot 1, row 1, ... with the gaps 0.25 + k / 256, k = 0, 1, ...
    from the left -- every gap is wider than the one before.  Frame 0 holds the slots' positions in row order (they are born into the
    slots 0 .. n - 1), frame 1 the rows' positions scattered over all 128 row indices.  4 x 2 m boxes along X, r_y = 0: the nearer pair
    is the better one under 'dist', 'bev' and '3d' alike, and every number is a multiple of 1 / 256 below 96: exact in float32.
    Slot i's nearest row is row i - 1 (i > 0), whose nearest slot is slot i - 1: only the leftmost pair that is left is mutual, so
    the rounds of phase 4 take ONE pair each and there are n of them -- the longest dependency the rule allows, and as many rounds as
    its loop has. """
    x, xs = -95.125, []
    for k in range(2 * n):
        xs.append(x)
        x += 0.25 + k / 256.0
    assert -96.0 < xs[0] and xs[-1] < 96.0
    order = np.random.default_rng(seed + n).permutation(D)
    first, second = padding(D), padding(D)
    for i in range(n):
        first[i] = row(0.5 + i / 256.0, xs[2 * i], 20.0, l=4.0)
        second[order[i]] = row(0.25 + i / 512.0, xs[2 * i + 1], 20.0, l=4.0)
    return np.stack([first, second])


LATTICE_X, LATTICE_Z = 2.125, 19.125          # the patch lies in the middle of a cell of full_house's grid, away from its cars


# With the shift (0.125, 0.0625) a slot's two nearest rows are its own column's and the column's to its left: slot 0 has one nearest row
# only, and column by column the serial rule has no choice -- the tie rule changes the rounds, not the matches.  Shifted the other way the
# first slot of the order has two equal rows that are both free, and whichever it takes decides every match to its right
BACK_SHIFT = (-0.125, 0.0625)


def lattice_car(k, dx=0.0, dz=0.0):
    return row(0.5 + k / 256.0, LATTICE_X + 0.25 * (k % 16) + dx, LATTICE_Z + 0.25 * (k // 16) + dz, l=4.0)


def lattice(nT, nR, seed=LATTICE_SEED, shift=(0.125, 0.0625)):
    """ 4 x 2 m cars, r_y = 0, on a 16-wide lattice of pitch 0.25 m: every car overlaps every other.
    frame 0   the first nT cars in row order: the slots 0 .. nT - 1
    frame 1   the first nR cars, moved by `shift`, in a seeded order, padding behind: every pair passes the gate, so the chunks of
              phase 3 are full, equal candidates abound and the rounds of phase 4 take many pairs each
    frame 2   nR rows on full_house's 8 m grid: nothing is a candidate -- a table line left over from frame 1 would be one
    frame 3   frame 1 again, against slots that have moved, missed a frame, and (nT < 128) the cars born in frame 2 """
    order = np.random.default_rng(seed + 128 * nT + nR).permutation(nR)
    first, moved, grid = padding(D), padding(D), padding(D)
    for k in range(nT):
        first[k] = lattice_car(k)
    for k in range(nR):
        moved[order[k]] = lattice_car(k, shift[0], shift[1])
        grid[k] = row(0.5 + k / 256.0, 8.0 * (k % 16), 16.0 + 8.0 * (k // 16), l=4.0)
    return np.stack([first, moved, grid, moved])


def edge_targets(nR):
    """ the pair indices p = a * nR + c on both sides of every chunk edge of 128 x nR pairs, the first pair and the last """
    pairs = D * nR
    edges = range(CHUNK, pairs, CHUNK)
    return sorted({0, pairs - 1} | {b - 1 for b in edges} | set(edges))


def boundary(nR, seed=BOUNDARY_SEED):
    """ the complement of the lattice: 128 cars on full_house's 8 m grid, each a candidate for its own slot and for no other, so that
    the gate leaves one survivor per slot -- and the row order of every frame is chosen so that these decisive pairs sit ON the edges of
    phase 3's chunks: pair p = a * nR + c (the a-th slot, the c-th live row) is a match for p = 4095 | 4096, 8191 | 8192, ..., for the
    first pair and for the last.  A pair dropped, doubled or read from the wrong chunk at an edge loses a track.
    frame 0   the cars in row order: slot k is car k
    frame f   nR of the cars (nR = 127: another car is hidden in every frame, so the lists' lengths differ and the edges fall inside a
              slot's line), padding behind; the cars of the edges at the row their pair needs, the others in a seeded order.  Two pairs
              that share a slot or a row go to different frames """
    rng = np.random.default_rng(seed + nR)
    wanted = []                                              # per frame {car: row}
    for p in edge_targets(nR):
        a, c = divmod(p, nR)
        for frame in wanted:
            if a not in frame and c not in frame.values():
                frame[a] = c
                break
        else:
            wanted.append({a: c})
    car = lambda k: row(0.5 + k / 256.0, 8.0 * (k % 16), 16.0 + 8.0 * (k // 16), l=4.0)  # noqa: E731
    out = [np.stack([car(k) for k in range(D)])]
    for f, at in enumerate(wanted):
        hidden = [k for k in range(100 + 3 * f, D) if k not in at][:D - nR]      # (never the same car twice in a row: nobody dies)
        others = [k for k in rng.permutation(D) if k not in at and k not in hidden]
        free = [c for c in range(nR) if c not in at.values()]
        frame = padding(D)
        for k, c in list(at.items()) + list(zip(others, free)):
            frame[c] = car(int(k))
        out.append(frame)
    return np.stack(out)


def turned_crowd(seed=CROWD_SEED):
    """ 128 cars in a patch of 8 x 5 m with headings from all directions and a car's sizes, seen three times with 10 cm and 0.05 rad of
    noise, the rows of every frame in a seeded order: rectangles that cross at every angle -- intersections of up to 8 vertices in all
    128 lanes of the clip.  A margin case: the seed is one for which no value lies within 1e-9 of the threshold or of another
    candidate's (tests/test_track_crowd_cpu.py asserts it) """
    rng = np.random.default_rng(seed)
    x, z = rng.uniform(0.0, 8.0, D) - 4.0, rng.uniform(0.0, 5.0, D) + 20.0
    ry, dims = rng.uniform(-math.pi, math.pi, D), rng.uniform([3.4, 1.5, 1.4], [4.8, 1.9, 1.8], (D, 3))
    out = []
    for _ in range(3):
        order, frame = rng.permutation(D), padding(D)
        for k in range(D):
            frame[order[k]] = row(rng.uniform(0.3, 1.0), x[k] + rng.normal(0.0, 0.1), z[k] + rng.normal(0.0, 0.1), dims[k][0], dims[k][1],
                                  ry[k] + rng.normal(0.0, 0.05), dims[k][2], 1.65 + rng.normal(0.0, 0.1), int(rng.integers(0, 4)))
        out.append(frame)
    return np.stack(out)


def crowd_options(metric):
    return options(metric, smooth=True, gains=CROWD_GAINS)


@functools.lru_cache(maxsize=None)
def scenes():
    """ {name: frames}; built once, never written to """
    out = {'chain_{}'.format(n): chain(n) for n in CHAIN_SIZES}
    out.update({'lattice_{}x{}'.format(nT, nR): lattice(nT, nR) for nT, nR in LATTICE_SIZES})
    out['lattice_128x128_back'] = lattice(128, 128, shift=BACK_SHIFT)
    out.update({'boundary_{}'.format(nR): boundary(nR) for nR in BOUNDARY_SIZES})
    out['turned_crowd'] = turned_crowd()
    return out


def cases():
    """ [(name, scene, options)] over the three metrics: the chains and the lattices are exact (r_y = 0, dyadic numbers: equal candidates
    are equal in every form), the turned crowd holds its margins """
    return [('{}_{}'.format(name, metric), name, crowd_options(metric) if name == 'turned_crowd' else options(metric))
            for name in scenes() for metric in T.METRICS]


def optimal_cases():
    return [(name, scene, P.optimal(opt)) for name, scene, opt in cases()]


def carried(name, records):
    """ a scene seen from a camera that moves by tests/track_ego_oracle.py's records (signed permutations about Y, dyadic translations):
    (frames, ego (N, 16)) """
    frames = scenes()[name]
    ego = E.cycle(records, len(frames))
    return E.carry(frames, ego), np.array(ego)


def drive_128():
    """ tests/track_oracle.py's sparse drive with padding behind its 16 rows: the same values in a frame of 128 """
    frames = O.drive(O.DRIVE_SEED)
    return np.concatenate([frames, np.full((frames.shape[0], D - frames.shape[1], 36), -1.0, np.float32)], axis=1)


# ---------------------------------------------------------------------------------------------------- references, computed once
def key_of(opt):
    return tuple(sorted((k, v) for k, v in opt.items()))


@functools.lru_cache(maxsize=None)
def _oracle(scene, key):
    opt = dict(key)
    values, matrices = [], []
    if opt.get('assign') == 'optimal':
        res = P.track(scenes()[scene], opt, values=values, matrices=matrices)
    else:                                                    # (O.track with the values of every frame in a list of their own)
        frames, st, steps = scenes()[scene], O.empty(), []
        for f in frames:
            values.append([])
            steps.append(O.step(st, f, opt, values[-1]))
        res = (np.array([s[0] for s in steps], np.float32).reshape(frames.shape), np.array([s[1] for s in steps], np.int32),
               np.array([s[2] for s in steps], np.int32), st)
    return res, values, matrices


def oracle(scene, opt):
    """ ((rows, ids, hits, state), per frame the (value, slot, row) of every pair, per frame (cost, slots, rows, pairs) -- optimal only)
    of the loop-written oracle; computed once per scene and option, shared, not to be written to """
    return _oracle(scene, key_of(opt))


@functools.lru_cache(maxsize=None)
def _host(scene, key):
    return T.track_rows_np(scenes()[scene], dict(key))


def host(scene, opt):
    """ (rows, ids, hits, state) of the NumPy form; computed once per scene and option """
    return _host(scene, key_of(opt))


@functools.lru_cache(maxsize=None)
def _trace(scene, key):
    opt = T.check_option(dict(key))
    state, out = T.empty_state(), []
    for rows in scenes()[scene]:
        occupied = state['id1'] != 0
        box = state['box'].copy()
        box[0:3, occupied] = box[0:3, occupied] + box[7:10, occupied]
        valid = (rows[:, 14] >= 0.0) & ~np.isnan(rows[:, T.ROW_COLS]).any(axis=1)
        keys = []
        T.step_np(state, rows, opt, keys)
        out.append({'keys': keys[0], 'occupied': occupied, 'valid': valid, 'box': box, 'rows': rows})
    return out


def trace(scene, opt):
    """ per frame of the NumPy form: the candidate table, the occupied slots and the live rows it was built for, the predicted state """
    return _trace(scene, key_of(opt))


# ---------------------------------------------------------------------------------------------------- what a frame reaches
def chunk_fill(frame):
    """ phase 3's gate, counted with its formula: ddx^2 + ddz^2 <= (rad_t + rad_r)^2 (1 + 1/32)^2 with rad the half diagonal, over the
    pairs p = a * nR + c of the listed slots and rows in chunks of 4096 -> [(pairs, survivors)] per chunk """
    box, rows = frame['box'], frame['rows'].astype(np.float64)
    ts, ds = np.flatnonzero(frame['occupied']), np.flatnonzero(frame['valid'])
    if ts.size == 0 or ds.size == 0:
        return []
    t, d = np.repeat(ts, ds.size), np.tile(ds, ts.size)
    rad_t = np.sqrt((box[6][t] / 2.0) ** 2 + (box[5][t] / 2.0) ** 2)
    rad_r = np.sqrt((rows[d, 18] / 2.0) ** 2 + (rows[d, 17] / 2.0) ** 2)
    ddx, ddz = box[0][t] - rows[d, 19], box[2][t] - rows[d, 21]
    passed = ~(ddx * ddx + ddz * ddz > (rad_t + rad_r) ** 2 * GATE_SLACK)
    return [(int(passed[a:a + CHUNK].size), int(passed[a:a + CHUNK].sum())) for a in range(0, passed.size, CHUNK)]


def most_vertices(frame):
    """ the largest vertex count of a slot's predicted rectangle clipped by a row's, over the frame's candidates (the oracle's clip) """
    box, rows, most = frame['box'], frame['rows'].astype(np.float64), 0
    for t, d in zip(*np.nonzero(np.isfinite(frame['keys']))):
        poly = corners(box[6][t], box[5][t], box[0][t], box[2][t], box[3][t])
        g = corners(rows[d, 18], rows[d, 17], rows[d, 19], rows[d, 21], rows[d, 32])
        for e in range(4):
            poly = clip(poly, g[e], g[(e + 1) % 4])
        most = max(most, len(poly))
    return most


# ---------------------------------------------------------------------------------------------------- phase 4, as track.hip states it
def bit(lo, hi, k):
    return ((lo >> k) if k < 64 else (hi >> (k - 64))) & 1


def ballot(flags):
    """ the two wavefronts' ballots: (threads 0 .. 63, threads 64 .. 127) """
    lo = sum(1 << k for k in range(64) if flags[k])
    hi = sum(1 << k for k in range(64) if flags[64 + k])
    return lo, hi


def phase4_rounds(keys, slots=None, rows=None, fault=None):
    """ The greedy phase 4 of csrc/track.hip, statement for statement, the 128 threads one after the other between its barriers: thread
    tid is slot tid and row tid and carries bd (the slot's best free row), bt (the row's best open slot), scan_line and scan_column
    (whether it looks again), and every thread keeps the same four 64-bit masks free_lo / free_hi (rows) and open_lo / open_hi (slots);
    a round takes the pairs that name each other, and the loop ends after min(slots, rows) rounds or when a round closes nothing.
    keys: the frame's candidate table (128, D) of utils/track.track_rows_np(..., keys_out=...); slots, rows: the occupied slots and the
    live rows (default: those with a candidate -- the others never take part).
    fault: None, or one of three deliberately wrong variants -- 'never_rescans', 'larger_row' (equal keys go to the larger row),
    'no_hi_masks' (the masks of the indices from 64 on are never updated).
    -> (the matches [(slot, row)] in slot order, per round the pairs it took) """
    assert fault in (None, 'never_rescans', 'larger_row', 'no_hi_masks')
    keys = np.asarray(keys, np.float64)
    finite = np.isfinite(keys)
    tlist = sorted(int(t) for t in (np.flatnonzero(finite.any(axis=1)) if slots is None else slots))
    rlist = sorted(int(d) for d in (np.flatnonzero(finite.any(axis=0)) if rows is None else rows))
    tab = keys.tolist()
    nT, nR = len(tlist), len(rlist)
    threads = range(T.MAX_TRACKS)
    is_slot, is_row = [t in set(tlist) for t in threads], [d in set(rlist) for d in threads]
    open_, unmatched, scan_line, scan_column = list(is_slot), list(is_row), list(is_slot), list(is_row)
    free_lo = free_hi = open_lo = open_hi = MASK
    bd, bt = [-1] * len(threads), [-1] * len(threads)
    mrow, mslot = [-1] * len(threads), [-1] * len(threads)
    taken = []
    for _ in range(min(nT, nR)):
        for tid in threads:
            if open_[tid] and scan_line[tid]:
                bkey, bd[tid] = math.inf, -1
                for d in rlist:
                    key = tab[tid][d]
                    better = key < bkey or (fault == 'larger_row' and key == bkey and key < math.inf)
                    if bit(free_lo, free_hi, d) and better:
                        bkey, bd[tid] = key, d
                scan_line[tid] = False
            if unmatched[tid] and scan_column[tid]:
                bkey, bt[tid] = math.inf, -1
                for t in tlist:
                    key = tab[t][tid]
                    if bit(open_lo, open_hi, t) and key < bkey:
                        bkey, bt[tid] = key, t
                scan_column[tid] = False
        s_bt = [bt[tid] if unmatched[tid] else -1 for tid in threads]
        # (barrier)
        take = [open_[tid] and bd[tid] >= 0 and s_bt[bd[tid]] == tid for tid in threads]
        for tid in threads:
            if take[tid]:
                open_[tid] = False
                mrow[tid], mslot[bd[tid]] = bd[tid], tid
        closed_lo, closed_hi = ballot(take)
        # (barrier)
        for tid in threads:
            if unmatched[tid] and mslot[tid] >= 0:
                unmatched[tid] = False
        gone_lo, gone_hi = ballot([is_row[tid] and not unmatched[tid] for tid in threads])
        # (barrier)
        if (closed_lo | closed_hi) == 0:
            break
        taken.append([(tid, bd[tid]) for tid in threads if take[tid]])
        open_lo, free_lo = open_lo & ~closed_lo & MASK, ~gone_lo & MASK
        if fault != 'no_hi_masks':
            open_hi, free_hi = open_hi & ~closed_hi & MASK, ~gone_hi & MASK
        if fault != 'never_rescans':
            for tid in threads:
                if open_[tid] and bd[tid] >= 0 and not bit(free_lo, free_hi, bd[tid]):
                    scan_line[tid] = True
                if unmatched[tid] and bt[tid] >= 0 and not bit(open_lo, open_hi, bt[tid]):
                    scan_column[tid] = True
    return [(t, mrow[t]) for t in threads if mrow[t] >= 0], taken
