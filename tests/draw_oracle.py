"""
The --save-images picture of DESIGN.md section 4.14 as plain loops: stepping lines, one pixel at a time, '{:.2f}'.format for the caption
text, math.sin / math.cos for the rotation.  The yardstick for utils/visualization.py (vectorised NumPy) and csrc/draw.hip (gpp_draw_build,
gpp_draw_raster); it shares nothing with them but the glyph table, which is data.

  build(rows, P, thr)        -> (n, records): the ordered primitive records of one image, each a list of 16 Python ints (include/gpp.h)
  real_endpoints(rows, P, thr)-> per record the real-valued coordinates its integers were truncated from (None where there are none)
  rasterise(frame, records)  -> (2h, w, 3) uint8
"""
import math
import struct

import numpy as np

from keras_retinanet_3D.utils.visualization import GLYPH_CHARS, GLYPH_ROWS

NONE, LINE, DASHED, RECT, CIRCLE, CAPTION = 0, 1, 2, 3, 4, 5
LIMIT = float(2 ** 20)
BOX_COLORS = [(0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)]
YELLOW = (0, 255, 255)
UP = [(0, -4), (-4, 4), (4, 4)]
SQ = [(-4, -4), (4, -4), (4, 4), (-4, 4)]
DOWN = [(0, 4), (-4, -4), (4, -4)]
# reference visualization.py:335-386: (corner, corner, dashed) per orientation class, in drawing order
S, D = False, True
EDGE_TABLE = {
    0: [(2, 3, D), (3, 7, D), (7, 6, S), (6, 2, S), (0, 3, D), (1, 2, S), (4, 7, S), (5, 6, S), (0, 1, S), (1, 5, S), (5, 4, S), (4, 0, S)],
    1: [(2, 3, D), (3, 7, S), (7, 6, S), (6, 2, D), (0, 3, S), (1, 2, D), (4, 7, S), (5, 6, S), (0, 1, S), (1, 5, S), (5, 4, S), (4, 0, S)],
    2: [(2, 3, S), (3, 7, S), (7, 6, S), (6, 2, S), (0, 3, D), (1, 2, S), (4, 7, S), (5, 6, S), (0, 1, D), (1, 5, S), (5, 4, S), (4, 0, D)],
    3: [(2, 3, S), (3, 7, S), (7, 6, S), (6, 2, S), (0, 3, S), (1, 2, D), (4, 7, S), (5, 6, S), (0, 1, D), (1, 5, D), (5, 4, S), (4, 0, S)],
}


def ok(v):
    return math.isfinite(v) and abs(v) < LIMIT


def s32(v):
    return struct.unpack('<i', struct.pack('<I', v & 0xffffffff))[0]


def record(kind, picture, x0, y0, x1, y1, color, bbox, text=''):
    codes = [GLYPH_CHARS.index(ch) for ch in text] + [0] * (20 - len(text))
    words = [s32(codes[4 * i] | codes[4 * i + 1] << 8 | codes[4 * i + 2] << 16 | codes[4 * i + 3] << 24) for i in range(5)]
    return [kind, picture, x0, y0, x1, y1, color[0] | color[1] << 8 | color[2] << 16] + list(bbox) + words


def line(picture, p, q, color, dashed):
    g = 1 if dashed else 0
    return record(DASHED if dashed else LINE, picture, p[0], p[1], q[0], q[1], color,
                  (min(p[0], q[0]) - g, min(p[1], q[1]) - g, max(p[0], q[0]) + g, max(p[1], q[1]) + g))


def value_text(v):
    v = float(np.float32(v))
    if not math.isfinite(v) or abs(v) >= 1e6:
        return '-'
    return '{:.2f}'.format(v)


def label_text(v):
    v = float(v)
    if not math.isfinite(v) or abs(v) >= 1e6:
        return '-'
    return '%d' % int(v)


def hsv(k, n):
    i, m = (6 * k) // n, (6 * k) % n
    up, down = (255 * m) // n, (255 * (n - m)) // n
    return [(255, up, 0), (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down)][i % 6]


def corners_real(row, P):
    """ the eight projected corners as real numbers [(u, v)], or None where no cuboid is drawn """
    pose = [float(v) for v in row[16:25]]
    if not all(math.isfinite(v) for v in pose):
        return None
    h, w, l = pose[0:3]
    loc, r = pose[3:6], pose[6:9]
    theta = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta > 3.2:
        return None
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if theta > 0.0:
        k = [r[0] / theta, r[1] / theta, r[2] / theta]
        c, s = math.cos(theta), math.sin(theta)
        K = [[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]]
        for i in range(3):
            for j in range(3):
                R[i][j] = c * (1.0 if i == j else 0.0) + (1.0 - c) * k[i] * k[j] + s * K[i][j]
    xs = [l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2]
    ys = [0.0, 0.0, 0.0, 0.0, -h, -h, -h, -h]
    zs = [w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2]
    out = []
    for c8 in range(8):
        X = [R[i][0] * xs[c8] + R[i][1] * ys[c8] + R[i][2] * zs[c8] + loc[i] for i in range(3)]
        x = [float(P[i][0]) * X[0] + float(P[i][1]) * X[1] + float(P[i][2]) * X[2] + float(P[i][3]) for i in range(3)]
        if not x[2] > 0.0:
            return None
        u, v = x[0] / x[2], x[1] / x[2]
        if not (ok(u) and ok(v)):
            return None
        out.append((u, v))
    return out


def selected(rows, thr):
    thr = np.float32(thr)
    return [d for d in range(len(rows)) if np.float32(rows[d][12]) > thr]


def build(rows, P, thr=0.4, real=None):
    """ real: an optional list that receives, per record, the real-valued (x0, y0, x1, y1) behind a cuboid edge's integers (else None) """
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 36)
    sel = selected(rows, thr)
    n = len(sel)
    recs = [[0] * 16 for _ in range(26 * n)]
    reals = [None] * (26 * n)
    for k, d in enumerate(sel):
        row = [float(v) for v in rows[d]]
        o = int(row[14]) if ok(row[14]) and 0 <= int(row[14]) <= 3 else -1
        top, marks, bottom = 3 * k, 3 * n + 10 * k, 13 * n + 13 * k
        if o >= 0 and all(ok(v) for v in row[0:4]):
            x1, y1, x2, y2 = (int(v) for v in row[0:4])
            xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
            recs[top] = record(RECT, 0, xa, ya, xb, yb, BOX_COLORS[o], (xa - 1, ya - 1, xb + 1, yb + 1))
        if ok(row[4]) and ok(row[5]):
            x, y = int(row[4]), int(row[5])
            recs[top + 1] = record(CIRCLE, 0, x, y, 0, 0, YELLOW, (x - 4, y - 4, x + 4, y + 4))
        if ok(row[0]) and ok(row[1]):
            x, y = int(row[0]), int(row[1]) - 10
            for slot, picture, value in ((top + 2, 0, rows[d][12]), (bottom, 1, rows[d][15])):
                text = label_text(row[13]) + ': ' + value_text(value)
                recs[slot] = record(CAPTION, picture, x, y, len(text), 0, (0, 0, 0), (x - 1, y - 7, x + 6 * len(text) - 1, y + 1), text)
        slot = marks
        for col, shape in ((6, UP), (8, SQ), (10, DOWN)):
            if ok(row[col]) and ok(row[col + 1]):
                cx, cy = int(row[col]), int(row[col + 1])
                pts = [(cx + dx, cy + dy) for dx, dy in shape]
                for i in range(len(pts)):
                    recs[slot + i] = line(0, pts[i], pts[(i + 1) % len(pts)], YELLOW, False)
            slot += len(shape)
        uv = corners_real(row, P) if o >= 0 else None
        if uv is not None:
            color = hsv(k, n)
            for e, (a, b, dashed) in enumerate(EDGE_TABLE[o]):
                recs[bottom + 1 + e] = line(1, (int(uv[a][0]), int(uv[a][1])), (int(uv[b][0]), int(uv[b][1])), color, dashed)
                reals[bottom + 1 + e] = (uv[a][0], uv[a][1], uv[b][0], uv[b][1])
    if real is not None:
        real[:] = reals
    return n, recs


# ------------------------------------------------------------------------------------------------ rasteriser
def put(img, x, y, color):
    if 0 <= x < img.shape[1] and 0 <= y < img.shape[0]:
        img[y, x, 0], img[y, x, 1], img[y, x, 2] = color


def step_line(img, x0, y0, x1, y1, color):
    dx, dy = x1 - x0, y1 - y0
    N = max(abs(dx), abs(dy))
    if N == 0:
        put(img, x0, y0, color)
        return
    H, W = img.shape[:2]
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    for i in range(N + 1):
        if abs(dx) >= abs(dy):
            x, y = x0 + i * sx, y0 + sy * ((2 * i * abs(dy) + N) // (2 * N))
        else:
            x, y = x0 + sx * ((2 * i * abs(dx) + N) // (2 * N)), y0 + i * sy
        put(img, x, y, color)


def dashed_line(img, x0, y0, x1, y1, color, gap=8):
    dist = math.sqrt(float((x1 - x0) ** 2 + (y1 - y0) ** 2))
    pts = []
    j = 0
    while float(j * gap) < dist:
        r = float(j * gap) / dist
        pts.append((int((x0 * (1 - r) + x1 * r) + .5), int((y0 * (1 - r) + y1 * r) + .5)))
        j += 1
    if len(pts) <= 1:
        return
    H, W = img.shape[:2]
    for j in range(1, len(pts), 2):
        a, b = pts[j - 1], pts[j]
        if max(a[0], b[0]) < 0 or max(a[1], b[1]) < 0 or min(a[0], b[0]) >= W or min(a[1], b[1]) >= H:
            continue                      # (a shortcut of the loop only: none of its pixels is inside)
        step_line(img, a[0], a[1], b[0], b[1], color)


def glyph_pixel(codes, cx, cy):
    if cy < 0 or cy >= 7 or cx < 0:
        return False
    i, c = cx // 6, cx % 6
    return i < len(codes) and c < 5 and GLYPH_ROWS[codes[i]][cy][c] == '#'


def paint(img, rec):
    kind, x0, y0, x1, y1 = rec[0], rec[2], rec[3], rec[4], rec[5]
    color = (rec[6] & 255, (rec[6] >> 8) & 255, (rec[6] >> 16) & 255)
    H, W = img.shape[:2]
    if kind == LINE:
        step_line(img, x0, y0, x1, y1, color)
    elif kind == DASHED:
        dashed_line(img, x0, y0, x1, y1, color)
    elif kind == RECT:
        for y in range(max(y0 - 1, 0), min(y1 + 1, H - 1) + 1):
            for x in range(max(x0 - 1, 0), min(x1 + 1, W - 1) + 1):
                if not (x0 + 1 <= x <= x1 - 1 and y0 + 1 <= y <= y1 - 1):
                    put(img, x, y, color)
    elif kind == CIRCLE:
        for dy in range(-4, 5):
            for dx in range(-4, 5):
                if 13 <= dx * dx + dy * dy <= 20:
                    put(img, x0 + dx, y0 + dy, color)
    elif kind == CAPTION:
        codes = []
        for i in range(min(max(x1, 0), 20)):
            codes.append(min((rec[11 + i // 4] >> (8 * (i % 4))) & 255, len(GLYPH_CHARS) - 1))
        for y in range(y0 - 7, y0 + 2):
            for x in range(x0 - 1, x0 + 6 * len(codes)):
                if any(glyph_pixel(codes, x - x0 + ddx, y - (y0 - 6) + ddy) for ddy in (-1, 0, 1) for ddx in (-1, 0, 1)):
                    put(img, x, y, (0, 0, 0))
        for y in range(y0 - 6, y0 + 1):
            for x in range(x0, x0 + 6 * len(codes)):
                if glyph_pixel(codes, x - x0, y - (y0 - 6)):
                    put(img, x, y, (255, 255, 255))
    elif kind != NONE:
        raise ValueError('unknown kind {}'.format(kind))


def rasterise(frame, recs):
    h = frame.shape[0]
    out = np.vstack((frame, frame))
    for rec in recs:
        rec = [int(v) for v in rec]
        if rec[0] != NONE:
            paint(out[h:] if rec[1] else out[:h], rec)
    return out


def composite(frame, rows, P, thr=0.4):
    return rasterise(frame, build(rows, P, thr)[1])
