"""
The --save-images composite of bin/run_network.py without OpenCV: the 2-D picture (boxes, keypoint markers, score captions) over the 3-D
picture (projected cuboids, residual captions), DESIGN.md section 4.14.

The reference draws with cv2 (anti-aliased rectangles, Hershey captions) and shuffles the cuboid colours with an unseeded RNG; this
module keeps its layout, order, colours, markers and solid / dashed edge pattern and defines the pixels itself, as integer rules that are
a pure function of the inputs.  Three forms of the rules agree byte for byte: tests/draw_oracle.py (plain loops), this module
(vectorised NumPy) and csrc/draw.hip (gpp_draw_build / gpp_draw_raster).  cv2's exact pixels are UNPINNED.

Two steps, as on the device:
  build_table(rows, P, score_threshold) -> (n, table (26 n, 16) int32)   the ordered primitive records of one image (include/gpp.h)
  raster(frame, table)                  -> (2h, w, 3) uint8               painter's order over two copies of the frame

The names the reference's bin/run_network.py imports (draw_box, draw_caption, draw_detections_with_keypoints, drawdashedline,
draw_3d_detections_from_pose) keep their signatures and draw in place on an ndarray.
"""

import numpy as np

# ------------------------------------------------------------------------------------------------ the record (include/gpp.h, gpp_draw_build)
PRIM_WORDS = 16            # int32 words per record
PRIMS_PER_DET = 26         # 3 (box, circle, caption) + 10 (marker lines) + 13 (caption, 12 edges)
KIND_NONE, KIND_LINE, KIND_DASHED, KIND_RECT, KIND_CIRCLE, KIND_CAPTION = 0, 1, 2, 3, 4, 5
F_KIND, F_PICTURE, F_X0, F_Y0, F_X1, F_Y1, F_COLOR, F_BX0, F_BY0, F_BX1, F_BY1, F_TEXT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
CAPTION_MAX = 20           # characters of a caption record (5 words)
COORD_LIMIT = 2.0 ** 20    # a primitive with a coordinate at or beyond it (or not finite) is skipped
ANGLE_LIMIT = 3.2          # a rotation vector longer than this draws no cuboid (the pose stage emits at most pi)
DASH_GAP = 8

# ------------------------------------------------------------------------------------------------ the font: 5 x 7, advance 6
GLYPH_CHARS = '0123456789.:- '
GLYPH_ROWS = (
    ('.###.', '#...#', '#..##', '#.#.#', '##..#', '#...#', '.###.'),   # 0
    ('..#..', '.##..', '..#..', '..#..', '..#..', '..#..', '.###.'),   # 1
    ('.###.', '#...#', '....#', '...#.', '..#..', '.#...', '#####'),   # 2
    ('.###.', '#...#', '....#', '..##.', '....#', '#...#', '.###.'),   # 3
    ('...#.', '..##.', '.#.#.', '#..#.', '#####', '...#.', '...#.'),   # 4
    ('#####', '#....', '####.', '....#', '....#', '#...#', '.###.'),   # 5
    ('..##.', '.#...', '#....', '####.', '#...#', '#...#', '.###.'),   # 6
    ('#####', '....#', '...#.', '..#..', '.#...', '.#...', '.#...'),   # 7
    ('.###.', '#...#', '#...#', '.###.', '#...#', '#...#', '.###.'),   # 8
    ('.###.', '#...#', '#...#', '.####', '....#', '...#.', '.##..'),   # 9
    ('.....', '.....', '.....', '.....', '.....', '.##..', '.##..'),   # .
    ('.....', '.##..', '.##..', '.....', '.##..', '.##..', '.....'),   # :
    ('.....', '.....', '.....', '#####', '.....', '.....', '.....'),   # -
    ('.....', '.....', '.....', '.....', '.....', '.....', '.....'),   # space
)
# bit (5 row + column) of GLYPH_BITS[g] is pixel (row, column) of glyph g, row 0 on top: the kernel's table (csrc/draw.hip kGlyphs)
GLYPH_BITS = tuple(sum(1 << (5 * r + c) for r in range(7) for c in range(5) if rows[r][c] == '#') for rows in GLYPH_ROWS)
_GLYPH_MASKS = np.array([[[ch == '#' for ch in row] for row in rows] for rows in GLYPH_ROWS], dtype=bool)      # (14, 7, 5)

# ------------------------------------------------------------------------------------------------ the picture's constants
BOX_COLORS = ((0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255))          # by orientation class (reference visualization.py:101)
MARK_COLOR = (0, 255, 255)
UP_TRIANGLE = ((0, -4), (-4, 4), (4, 4))                                   # :102-104
SQUARE = ((-4, -4), (4, -4), (4, 4), (-4, 4))
DOWN_TRIANGLE = ((0, 4), (-4, -4), (4, -4))
# the 12 cuboid edges in drawing order (:335-386; the corner pairs are the same for every orientation class) ...
EDGES = ((2, 3), (3, 7), (7, 6), (6, 2), (0, 3), (1, 2), (4, 7), (5, 6), (0, 1), (1, 5), (5, 4), (4, 0))
# ... and which of them are dashed, per orientation class
DASHED_EDGES = ((0, 1, 4), (0, 3, 5), (4, 8, 11), (5, 8, 9))
# corner k of the cuboid = R (CORNER_X[k] l/2, CORNER_Y[k] h, CORNER_Z[k] w/2) + location (utils.gpp_utils.cuboid_corners)
CORNER_X = (1, 1, -1, -1, 1, 1, -1, -1)
CORNER_Y = (0, 0, 0, 0, -1, -1, -1, -1)
CORNER_Z = (1, -1, -1, 1, 1, -1, -1, 1)


def edge_pattern():
    """ {orientation class: [(corner a, corner b, dashed)] * 12} """
    return {o: [(a, b, e in DASHED_EDGES[o]) for e, (a, b) in enumerate(EDGES)] for o in range(4)}


# ------------------------------------------------------------------------------------------------ numbers -> integers and text
def _coord_ok(*values):
    return all(np.isfinite(v) and abs(v) < COORD_LIMIT for v in values)


def format_value(v):
    """ the two-decimal text of a caption for float32 v: q = rint(double(v) * 100) half to even (the product is exact in float64, so this
    is '{:.2f}'.format(v)); '-' in front when signbit(v); '-' alone for a non-finite v or |v| >= 1e6 """
    v = float(np.float32(v))
    if not np.isfinite(v) or abs(v) >= 1e6:
        return '-'
    q = int(abs(np.rint(v * 100.0)))
    return ('-' if np.signbit(v) else '') + '{}.{:02d}'.format(q // 100, q % 100)


def format_label(label):
    """ '%d' of the label (truncated toward zero); '-' for a non-finite one or |label| >= 1e6 """
    label = float(label)
    if not np.isfinite(label) or abs(label) >= 1e6:
        return '-'
    return '{:d}'.format(int(label))


def hsv_color(k, n):
    """ HSV(k / n, 1, 1) * 255 truncated, in integers (matplotlib.colors.hsv_to_rgb's six sectors): sector i = 6k div n, m = 6k mod n,
    rising channel 255 m div n, falling channel 255 (n - m) div n """
    i, m = divmod(6 * k, n)
    up, down = 255 * m // n, 255 * (n - m) // n
    return ((255, up, 0), (down, 255, 0), (0, 255, up), (0, down, 255), (up, 0, 255), (255, 0, down))[i % 6]


def _pack(color):
    return int(color[0]) | int(color[1]) << 8 | int(color[2]) << 16


def _record(kind, picture, x0, y0, x1, y1, color, bbox, text=None):
    r = np.zeros(PRIM_WORDS, np.int64)
    r[:F_TEXT] = (kind, picture, x0, y0, x1, y1, color) + tuple(bbox)
    if text is not None:
        codes = np.zeros(CAPTION_MAX, np.uint8)
        codes[:len(text)] = [GLYPH_CHARS.index(ch) for ch in text]
        r[F_TEXT:] = codes.view('<u4')
    return (r & 0xffffffff).astype(np.uint32).view(np.int32)


def line_record(picture, p, q, color, dashed=False):
    x0, y0, x1, y1 = int(p[0]), int(p[1]), int(q[0]), int(q[1])
    g = 1 if dashed else 0          # (a dash sample of a negative coordinate truncates toward zero: one pixel beyond the endpoints' hull)
    return _record(KIND_DASHED if dashed else KIND_LINE, picture, x0, y0, x1, y1, _pack(color),
                   (min(x0, x1) - g, min(y0, y1) - g, max(x0, x1) + g, max(y0, y1) + g))


def rect_record(picture, x1, y1, x2, y2, color):
    xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    return _record(KIND_RECT, picture, xa, ya, xb, yb, _pack(color), (xa - 1, ya - 1, xb + 1, yb + 1))


def circle_record(picture, x, y, color):
    return _record(KIND_CIRCLE, picture, x, y, 0, 0, _pack(color), (x - 4, y - 4, x + 4, y + 4))


def caption_record(picture, x, y, text):
    if len(text) > CAPTION_MAX:
        raise ValueError('a caption holds at most {} characters, got {!r}'.format(CAPTION_MAX, text))
    bad = [ch for ch in text if ch not in GLYPH_CHARS]
    if bad:
        raise ValueError('the caption font has the characters {!r} only, got {!r}'.format(GLYPH_CHARS, text))
    return _record(KIND_CAPTION, picture, x, y, len(text), 0, 0, (x - 1, y - 7, x + 6 * len(text) - 1, y + 1), text)


def polyline_records(picture, cx, cy, offsets, color):
    pts = [(cx + dx, cy + dy) for dx, dy in offsets]
    return [line_record(picture, pts[i], pts[(i + 1) % len(pts)], color) for i in range(len(pts))]


def project_cuboid(row, P):
    """ the eight projected corners [(u, v)] of one row, or None where section 4.14 draws no cuboid: a non-finite pose column, a rotation
    vector longer than ANGLE_LIMIT, a corner at or behind the camera, a coordinate out of range """
    pose = np.asarray(row[16:25], dtype=np.float64)
    if not np.isfinite(pose).all():
        return None
    h, w, l = pose[0:3]
    r = pose[6:9]
    theta = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if theta > ANGLE_LIMIT:
        return None
    if theta > 0.0:
        k = r / theta
        c, s = np.cos(theta), np.sin(theta)
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        R = c * np.eye(3) + (1.0 - c) * np.outer(k, k) + s * K
    else:
        R = np.eye(3)
    X = np.stack([np.array(CORNER_X) * (l / 2), np.array(CORNER_Y) * h, np.array(CORNER_Z) * (w / 2)])          # (3, 8)
    X = R @ X + pose[3:6, None]
    x = np.asarray(P, dtype=np.float64) @ np.concatenate([X, np.ones((1, 8))], axis=0)
    if not (x[2] > 0.0).all():
        return None
    with np.errstate(all='ignore'):
        uv = x[:2] / x[2]
    if not (np.isfinite(uv).all() and (np.abs(uv) < COORD_LIMIT).all()):
        return None
    return [(int(uv[0, k]), int(uv[1, k])) for k in range(8)]


def select(rows, score_threshold):
    """ the indices of the rows with score > threshold (float32 comparison; a NaN score is not selected), in row order """
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 36)
    return np.nonzero(rows[:, 12] > np.float32(score_threshold))[0]


def build_table(rows, P, score_threshold=0.4):
    """ one image's pose rows (D, 36) + its calibration P (3, 4) in raw-image pixels -> (n, table (26 n, 16) int32): the primitive records of
    gpp_draw_build in painter's order.  Top picture: records [0, 3n) = box, circle, caption of every detection, [3n, 13n) = the ten marker
    lines of every detection; bottom picture: [13n, 26n) = caption and twelve edges of every detection.  A skipped primitive keeps its
    slot as KIND_NONE. """
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 36)
    sel = select(rows, score_threshold)
    n = len(sel)
    table = np.zeros((PRIMS_PER_DET * n, PRIM_WORDS), np.int32)
    for k, d in enumerate(sel):
        row = rows[d].astype(np.float64)
        o = int(row[14]) if _coord_ok(row[14]) and 0 <= int(row[14]) <= 3 else -1
        label = format_label(row[13]) + ': '
        anchor = (int(row[0]), int(row[1]) - 10) if _coord_ok(row[0], row[1]) else None
        top, marks, bottom = 3 * k, 3 * n + 10 * k, 13 * n + 13 * k
        if o >= 0 and _coord_ok(*row[0:4]):
            table[top] = rect_record(0, int(row[0]), int(row[1]), int(row[2]), int(row[3]), BOX_COLORS[o])
        if _coord_ok(row[4], row[5]):
            table[top + 1] = circle_record(0, int(row[4]), int(row[5]), MARK_COLOR)
        if anchor is not None:
            table[top + 2] = caption_record(0, anchor[0], anchor[1], label + format_value(rows[d, 12]))
            table[bottom] = caption_record(1, anchor[0], anchor[1], label + format_value(rows[d, 15]))
        for first, col, shape in ((0, 6, UP_TRIANGLE), (3, 8, SQUARE), (7, 10, DOWN_TRIANGLE)):
            if _coord_ok(row[col], row[col + 1]):
                recs = polyline_records(0, int(row[col]), int(row[col + 1]), shape, MARK_COLOR)
                table[marks + first:marks + first + len(recs)] = recs
        uv = project_cuboid(row, P) if o >= 0 else None
        if uv is not None:
            color = hsv_color(k, n)
            for e, (a, b) in enumerate(EDGES):
                table[bottom + 1 + e] = line_record(1, uv[a], uv[b], color, dashed=e in DASHED_EDGES[o])
    return n, table


# ------------------------------------------------------------------------------------------------ painting (vectorised)
def _paint_line(img, x0, y0, x1, y1, color):
    """ LINE: N = max(|dx|, |dy|); for i = 0 .. N the major coordinate is start + i sign, the minor one start + sign(dm) floor((2 i |dm| + N) / (2N)) """
    H, W = img.shape[:2]
    dx, dy = x1 - x0, y1 - y0
    x_major = abs(dx) >= abs(dy)
    N = max(abs(dx), abs(dy))
    if N == 0:
        if 0 <= x0 < W and 0 <= y0 < H:
            img[y0, x0] = color
        return
    a0, da, limit = (x0, dx, W) if x_major else (y0, dy, H)
    sa = 1 if da > 0 else -1
    # i with 0 <= a0 + i sa < limit
    lo, hi = (max(0, -a0), min(N, limit - 1 - a0)) if sa > 0 else (max(0, a0 - limit + 1), min(N, a0))
    if lo > hi:
        return
    i = np.arange(lo, hi + 1, dtype=np.int64)
    dm = dy if x_major else dx
    sm = (dm > 0) - (dm < 0)
    major = a0 + i * sa
    minor = (y0 if x_major else x0) + sm * ((2 * i * abs(dm) + N) // (2 * N))
    ok = (minor >= 0) & (minor < (H if x_major else W))
    xs, ys = (major[ok], minor[ok]) if x_major else (minor[ok], major[ok])
    img[ys, xs] = color


def dash_samples(x0, y0, x1, y1, gap=DASH_GAP):
    """ the reference's drawdashedline samples: i = 0, gap, 2 gap, ... < dist, r = i / dist, int(p (1 - r) + q r + .5) (float64, in this order) """
    dist = np.sqrt(np.float64((x1 - x0) ** 2 + (y1 - y0) ** 2))
    if not dist > 0.0:
        return np.zeros((0, 2), np.int64)
    i = np.arange(int(np.ceil(dist / gap)), dtype=np.float64) * gap
    i = i[i < dist]
    r = i / dist
    xs = (x0 * (1.0 - r) + x1 * r) + .5
    ys = (y0 * (1.0 - r) + y1 * r) + .5
    return np.stack([np.trunc(xs), np.trunc(ys)], axis=1).astype(np.int64)


def _paint_dashed(img, x0, y0, x1, y1, color, gap=DASH_GAP):
    H, W = img.shape[:2]
    pts = dash_samples(x0, y0, x1, y1, gap)
    for j in range(1, len(pts), 2):
        (ax, ay), (bx, by) = pts[j - 1], pts[j]
        if max(ax, bx) < 0 or max(ay, by) < 0 or min(ax, bx) >= W or min(ay, by) >= H:
            continue
        _paint_line(img, int(ax), int(ay), int(bx), int(by), color)


def _fill(img, xa, ya, xb, yb, color):
    H, W = img.shape[:2]
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)
    if xa <= xb and ya <= yb:
        img[ya:yb + 1, xa:xb + 1] = color


def _paint_rect(img, x1, y1, x2, y2, color):
    """ RECT, thickness 2: [x1 - 1, x2 + 1] x [y1 - 1, y2 + 1] without [x1 + 1, x2 - 1] x [y1 + 1, y2 - 1] """
    if x2 - x1 < 2 or y2 - y1 < 2:
        _fill(img, x1 - 1, y1 - 1, x2 + 1, y2 + 1, color)
        return
    _fill(img, x1 - 1, y1 - 1, x2 + 1, y1, color)
    _fill(img, x1 - 1, y2, x2 + 1, y2 + 1, color)
    _fill(img, x1 - 1, y1 + 1, x1, y2 - 1, color)
    _fill(img, x2, y1 + 1, x2 + 1, y2 - 1, color)


_CIRCLE_OFFSETS = np.array([(dx, dy) for dy in range(-4, 5) for dx in range(-4, 5) if 13 <= dx * dx + dy * dy <= 20], dtype=np.int64)


def _paint_mask(img, x, y, mask, color):
    """ mask (rows, columns) of booleans with its top-left pixel at (x, y) """
    H, W = img.shape[:2]
    mh, mw = mask.shape
    xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + mw, W), min(y + mh, H)
    if xa < xb and ya < yb:
        img[ya:yb, xa:xb][mask[ya - y:yb - y, xa - x:xb - x]] = color


def _paint_circle(img, x, y, color):
    H, W = img.shape[:2]
    xs, ys = _CIRCLE_OFFSETS[:, 0] + x, _CIRCLE_OFFSETS[:, 1] + y
    ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    img[ys[ok], xs[ok]] = color


def _paint_caption(img, x, y, codes):
    """ CAPTION: pass 1 every glyph pixel dilated 3 x 3 in black, pass 2 the glyph pixels in white; (x, y) = bottom-left corner of the first glyph """
    if len(codes) == 0:
        return
    glyphs = np.zeros((7 + 2, 6 * len(codes) + 2), dtype=bool)          # one pixel of margin all round
    for i, g in enumerate(codes):
        glyphs[1:8, 1 + 6 * i:1 + 6 * i + 5] = _GLYPH_MASKS[g]
    dilated = np.zeros_like(glyphs)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dilated[max(dy, 0):glyphs.shape[0] + min(dy, 0), max(dx, 0):glyphs.shape[1] + min(dx, 0)] |= \
                glyphs[max(-dy, 0):glyphs.shape[0] + min(-dy, 0), max(-dx, 0):glyphs.shape[1] + min(-dx, 0)]
    _paint_mask(img, x - 1, y - 7, dilated, (0, 0, 0))
    _paint_mask(img, x - 1, y - 7, glyphs, (255, 255, 255))


def _unpack(word):
    word = int(word) & 0xffffffff
    return (word & 255, (word >> 8) & 255, (word >> 16) & 255)


def paint(img, record):
    """ one record onto img (h, w, 3) uint8, in place """
    rec = [int(v) for v in record[:F_TEXT]]
    kind, x0, y0, x1, y1, color = rec[F_KIND], rec[F_X0], rec[F_Y0], rec[F_X1], rec[F_Y1], _unpack(rec[F_COLOR])
    if kind == KIND_LINE:
        _paint_line(img, x0, y0, x1, y1, color)
    elif kind == KIND_DASHED:
        _paint_dashed(img, x0, y0, x1, y1, color)
    elif kind == KIND_RECT:
        _paint_rect(img, x0, y0, x1, y1, color)
    elif kind == KIND_CIRCLE:
        _paint_circle(img, x0, y0, color)
    elif kind == KIND_CAPTION:
        codes = np.ascontiguousarray(record[F_TEXT:], dtype=np.int32).view(np.uint8)[:min(max(x1, 0), CAPTION_MAX)]
        _paint_caption(img, x0, y0, np.minimum(codes, len(GLYPH_CHARS) - 1))
    elif kind != KIND_NONE:
        raise ValueError('unknown primitive kind {}'.format(kind))


def raster(frame, table):
    """ the composite (2h, w, 3) of one frame (h, w, 3) uint8 and its primitive table, painter's order """
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError('the frame must be (h, w, 3) uint8, got {} {}'.format(frame.shape, frame.dtype))
    h = frame.shape[0]
    out = np.vstack((frame, frame))
    pictures = (out[:h], out[h:])
    for record in np.asarray(table, dtype=np.int32).reshape(-1, PRIM_WORDS):
        if record[F_KIND] != KIND_NONE:
            paint(pictures[1 if record[F_PICTURE] else 0], record)
    return out


# ------------------------------------------------------------------------------------------------ whole composites
def rows_from_detections(det):
    """ the columns of a pose row that the picture reads (0-24) from the dict of gpp_utils.recover_pose / detections_from_rows """
    n = len(det['scores'])
    rows = np.zeros((n, 36), np.float32)
    rows[:, 0:12] = np.asarray(det['boxes'], dtype=np.float32).reshape(n, 12)
    rows[:, 12] = det['scores']
    rows[:, 13] = det['labels']
    rows[:, 14] = det['orientations']
    rows[:, 15] = det['residuals']
    rows[:, 16:19] = det['dimensions']
    rows[:, 19:22] = det['locations']
    rows[:, 22:25] = det['angles']
    return rows


def composite_from_rows(raw_image, rows_b, count, P, score_threshold=0.4):
    """ the composite of one image from its rows of the device pose stage (the first `count` rows; None = all of them) """
    rows = np.asarray(rows_b, dtype=np.float32).reshape(-1, 36)
    rows = rows if count is None else rows[:int(count)]
    return raster(raw_image, build_table(rows, P, score_threshold)[1])


def composite(raw_image, det, P, score_threshold=0.4):
    """ reference run_network.py:334-338 for one image: det = the dict of gpp_utils.recover_pose, P = the calibration in raw-image pixels
    (after :115).  Returns the (2h, w, 3) uint8 picture; raw_image is not modified. """
    return composite_from_rows(raw_image, rows_from_detections(det), None, P, score_threshold)


def write_png(path, bgr):
    """ a BGR uint8 image as a PNG file (what cv2.imwrite does for the reference; the inverse of utils.image.read_image_bgr) """
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(np.asarray(bgr, dtype=np.uint8)[:, :, ::-1])).save(path, format='PNG')


# ------------------------------------------------------------------------------------------------ the reference's names (in place)
def _check_canvas(image):
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('the image must be an (h, w, 3) uint8 ndarray')


def _caption_text(label, value, label_to_name):
    return (label_to_name(label) if label_to_name else format_label(label)) + ': ' + format_value(value)


def draw_box(image, box, color, thickness=2):
    """ RECT of int(box[0:4]) (thickness 2 is the only one section 4.14 defines) """
    _check_canvas(image)
    if thickness != 2:
        raise ValueError('draw_box draws thickness 2 only')
    b = np.asarray(box, dtype=np.float64)
    if _coord_ok(*b[:4]):
        paint(image, rect_record(0, int(b[0]), int(b[1]), int(b[2]), int(b[3]), color))


def draw_caption(image, box, caption):
    """ CAPTION of the text at (int(box[0]), int(box[1]) - 10); the font has the characters of GLYPH_CHARS """
    _check_canvas(image)
    b = np.asarray(box, dtype=np.float64)
    if _coord_ok(b[0], b[1]):
        paint(image, caption_record(0, int(b[0]), int(b[1]) - 10, caption))


def drawdashedline(img, pt1, pt2, color, thickness=1, gap=8):
    """ DASHED(pt1, pt2) (thickness 1 is the only one section 4.14 defines) """
    _check_canvas(img)
    if thickness != 1:
        raise ValueError('drawdashedline draws thickness 1 only')
    _paint_dashed(img, int(pt1[0]), int(pt1[1]), int(pt2[0]), int(pt2[1]), tuple(int(c) for c in color), gap)


def draw_detections_with_keypoints(image, boxes, scores, labels, orientations, label_to_name=None, score_threshold=0.5):
    """ the top picture, in place (reference visualization.py:89-127) """
    _check_canvas(image)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 12)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    sel = np.nonzero(scores > np.float32(score_threshold))[0]
    marks = []
    for d in sel:
        b = boxes[d]
        o = int(orientations[d])
        if 0 <= o <= 3:
            draw_box(image, b[:4], BOX_COLORS[o])
        if _coord_ok(b[4], b[5]):
            paint(image, circle_record(0, int(b[4]), int(b[5]), MARK_COLOR))
        for col, shape in ((6, UP_TRIANGLE), (8, SQUARE), (10, DOWN_TRIANGLE)):
            if _coord_ok(b[col], b[col + 1]):
                marks += polyline_records(0, int(b[col]), int(b[col + 1]), shape, MARK_COLOR)
        draw_caption(image, b, _caption_text(labels[d], scores[d], label_to_name))
    for rec in marks:
        paint(image, rec)


def draw_3d_detections_from_pose(image, boxes, orientations, residuals, scores, labels, locations, angles, dimensions, P,
                                 label_to_name=None, score_threshold=0.5):
    """ the bottom picture, in place (reference visualization.py:281-388; the colours are not shuffled) """
    _check_canvas(image)
    boxes = np.asarray(boxes, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    sel = np.nonzero(scores > np.float32(score_threshold))[0]
    n = len(sel)
    for k, d in enumerate(sel):
        draw_caption(image, boxes[d], _caption_text(labels[d], residuals[d], label_to_name))
        o = int(orientations[d])
        row = np.zeros(36, np.float32)
        row[16:19], row[19:22], row[22:25] = dimensions[d], locations[d], angles[d]
        uv = project_cuboid(row, P) if 0 <= o <= 3 else None
        if uv is not None:
            color = hsv_color(k, n)
            for e, (a, b) in enumerate(EDGES):
                paint(image, line_record(0, uv[a], uv[b], color, dashed=e in DASHED_EDGES[o]))
