// The --save-images composite on gfx950 (MI355X): the 2-D picture (boxes, keypoint markers, score captions) over the 3-D picture
// (projected cuboids, residual captions), from the rows of gpp_pose_f32 and the raw uint8 frames.  DESIGN.md section 4.14 is the
// specification; utils/visualization.py (NumPy) and tests/draw_oracle.py (plain loops) are its two other forms, and the three agree byte
// for byte.  Layout, order, colours, markers and the solid / dashed edge pattern are the reference's
// (its keras_retinanet_3D/utils/visualization.py:89-127, :281-388 and bin/run_network.py:334-338); the pixels are this project's
// own integer rules -- cv2's anti-aliased rectangle and Hershey captions are UNPINNED, and the reference's colour shuffle is dropped.
//
// Two stages.
//   draw_build_kernel   one thread per detection, one workgroup per image (like pose_kernel): rows + P -> an ordered table of primitive
//                       records (kind, picture, integer endpoints, colour, bounding box, caption characters) and n per image.  float64,
//                       every operation separate (-ffp-contract=off).  Sine and cosine of the rotation angle are evaluated here, on
//                       [0, 3.2] only (the pose stage emits at most pi; a longer vector draws no cuboid): two-constant reduction by
//                       pi/2 and the two polynomial kernels, so no table-driven argument reduction, nothing indexed at run time, no scratch.
//   draw_raster_kernel  one workgroup per 64 x 4 tile of output pixels, one pixel per thread.  The image's records are examined 256 at a
//                       time, last chunk first; those whose bounding box meets the tile are compacted into LDS in their order (a prefix
//                       sum over ballots, no atomic append) and every thread walks that list backwards and takes the colour of the first
//                       record that covers its pixel -- painter's order without painting.  Coverage is closed form and exact integer
//                       arithmetic: a LINE pixel from its major coordinate, a DASHED pixel from the at most three dashes around its
//                       parameter along the line.  A tile that met no record is a copy in aligned 32-bit stores.  No atomic decides a colour:
//                       the bytes do not depend on timing, on the batch or on the tile size (section 4.4).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"

namespace {

constexpr int kBuildThreads = 128;
constexpr int kTileW = 64, kTileH = 4;
constexpr int kRasterThreads = kTileW * kTileH;
constexpr int kChunk = kRasterThreads;              // records examined per pass: one per thread
constexpr double kCoordLimit = 1048576.0;           // 2^20
constexpr double kAngleLimit = 3.2;
constexpr int kPerDet = GPP_DRAW_PRIMS_PER_DET;

// bit (5 row + column) of kGlyphs[g] is pixel (row, column) of glyph g of "0123456789.:- ", row 0 on top (utils/visualization.py GLYPH_BITS)
__device__ __constant__ uint64_t kGlyphs[14] = {
    0x3a33ae62eull, 0x3884210c4ull, 0x7c444422eull, 0x3a306422eull, 0x211f4a988ull, 0x3a3083c3full, 0x3a317844cull,
    0x08422221full, 0x3a317462eull, 0x1910f462eull, 0x18c000000ull, 0x00c6018c0ull, 0x0000f8000ull, 0x000000000ull};
constexpr uint32_t kDot = 10, kColon = 11, kMinus = 12, kSpace = 13;

struct Prim {
    int32_t kind, picture, x0, y0, x1, y1, color, bx0, by0, bx1, by1;
    uint32_t text[5];
};
static_assert(sizeof(Prim) == GPP_DRAW_PRIM_WORDS * 4, "a record is 16 words");

__device__ inline void store_prim(Prim* __restrict__ dst, const Prim& p)
{
    int4* d = reinterpret_cast<int4*>(dst);
    d[0] = make_int4(p.kind, p.picture, p.x0, p.y0);
    d[1] = make_int4(p.x1, p.y1, p.color, p.bx0);
    d[2] = make_int4(p.by0, p.bx1, p.by1, (int)p.text[0]);
    d[3] = make_int4((int)p.text[1], (int)p.text[2], (int)p.text[3], (int)p.text[4]);
}

__device__ inline Prim make_prim(int kind, int picture, int x0, int y0, int x1, int y1, int color, int bx0, int by0, int bx1, int by1)
{
    Prim p;
    p.kind = kind; p.picture = picture; p.x0 = x0; p.y0 = y0; p.x1 = x1; p.y1 = y1; p.color = color;
    p.bx0 = bx0; p.by0 = by0; p.bx1 = bx1; p.by1 = by1;
    p.text[0] = 0; p.text[1] = 0; p.text[2] = 0; p.text[3] = 0; p.text[4] = 0;
    return p;
}

__device__ inline Prim none_prim() { return make_prim(GPP_DRAW_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }

__device__ inline Prim line_prim(int picture, int x0, int y0, int x1, int y1, int color, bool dashed)
{
    const int g = dashed ? 1 : 0;          // a dash sample of a negative coordinate truncates toward zero: one pixel beyond the endpoints' hull
    return make_prim(dashed ? GPP_DRAW_DASHED : GPP_DRAW_LINE, picture, x0, y0, x1, y1, color,
                     min(x0, x1) - g, min(y0, y1) - g, max(x0, x1) + g, max(y0, y1) + g);
}

// finite and |v| < 2^20 (a NaN fails the comparison)
__device__ inline bool coord_ok(double v) { return fabs(v) < kCoordLimit; }

// ---------------------------------------------------------------------------------------------- caption text, in registers
struct Text { uint64_t lo, hi; uint32_t w2; int len; };

__device__ inline void put(Text& t, uint32_t code)
{
    const int p = t.len;
    if (p < 8) t.lo |= (uint64_t)code << (8 * p);
    else if (p < 16) t.hi |= (uint64_t)code << (8 * (p - 8));
    else if (p < GPP_DRAW_CAPTION_MAX) t.w2 |= code << (8 * (p - 16));
    if (p < GPP_DRAW_CAPTION_MAX) t.len = p + 1;
}

// decimal digits of v < 10^8 without leading zeros
__device__ inline void put_uint(Text& t, uint32_t v)
{
    bool started = false;
#pragma unroll
    for (uint32_t div = 10000000u; div >= 1u; div /= 10u) {
        const uint32_t dg = v / div;
        v -= dg * div;
        if (dg != 0u || started || div == 1u) { put(t, dg); started = true; }
    }
}

// "%d: " % label, then the value with two decimals: q = rint(double(v) * 100), half to even (the product is exact in float64)
__device__ inline Text caption_text(float label, float value)
{
    Text t = {0ull, 0ull, 0u, 0};
    const double lv = (double)label;
    if (!(fabs(lv) < 1e6)) put(t, kMinus);
    else {
        const int L = (int)lv;
        if (L < 0) put(t, kMinus);
        put_uint(t, (uint32_t)(L < 0 ? -L : L));
    }
    put(t, kColon); put(t, kSpace);
    const double dv = (double)value;
    if (!(fabs(dv) < 1e6)) put(t, kMinus);
    else {
        const uint32_t q = (uint32_t)fabs(rint(dv * 100.0));
        if (signbit(value)) put(t, kMinus);
        put_uint(t, q / 100u);
        put(t, kDot);
        put(t, (q % 100u) / 10u);
        put(t, q % 10u);
    }
    return t;
}

__device__ inline Prim caption_prim(int picture, int x, int y, const Text& t)
{
    Prim p = make_prim(GPP_DRAW_CAPTION, picture, x, y, t.len, 0, 0, x - 1, y - 7, x + 6 * t.len - 1, y + 1);
    p.text[0] = (uint32_t)t.lo; p.text[1] = (uint32_t)(t.lo >> 32); p.text[2] = (uint32_t)t.hi; p.text[3] = (uint32_t)(t.hi >> 32); p.text[4] = t.w2;
    return p;
}

// ---------------------------------------------------------------------------------------------- sine and cosine on [0, 3.2]
__device__ inline void sincos_small(double x, double& s, double& c)
{
    const double n = rint(x * 0.63661977236758134308);                                   // 0, 1 or 2 quarter turns
    const double y = (x - n * 1.57079632673412561417) - n * 6.07710050650619224932e-11;   // |y| <= pi/4 + 0.06
    const double z = y * y;
    const double sp = y + y * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double cp = 1.0 - 0.5 * z + z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const int q = (int)n;
    s = q == 0 ? sp : q == 1 ? cp : -sp;
    c = q == 0 ? cp : q == 1 ? -sp : -cp;
}

// HSV(k / n, 1, 1) * 255 truncated, in integers: sector i = 6k div n, m = 6k mod n
__device__ inline int hsv_color(int k, int n)
{
    const int i = (6 * k) / n, m = (6 * k) - i * n;
    const int up = (255 * m) / n, down = (255 * (n - m)) / n;
    int c0, c1, c2;
    switch (i % 6) {
    case 0: c0 = 255; c1 = up; c2 = 0; break;
    case 1: c0 = down; c1 = 255; c2 = 0; break;
    case 2: c0 = 0; c1 = 255; c2 = up; break;
    case 3: c0 = 0; c1 = down; c2 = 255; break;
    case 4: c0 = up; c1 = 0; c2 = 255; break;
    default: c0 = 255; c1 = 0; c2 = down; break;
    }
    return c0 | (c1 << 8) | (c2 << 16);
}

// a closed polyline of V vertices (offsets ox, oy from the centre) into V consecutive slots, or V empty slots
template <int V>
__device__ inline void marker(Prim* __restrict__ dst, bool ok, int cx, int cy, const int (&ox)[V], const int (&oy)[V], int color)
{
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int j = (i + 1) % V;
        store_prim(dst + i, ok ? line_prim(0, cx + ox[i], cy + oy[i], cx + ox[j], cy + oy[j], color, false) : none_prim());
    }
}

// the 26 records of one selected detection (rank k of n) of one image
__device__ inline void build_detection(const float* __restrict__ row, const double* __restrict__ P, int k, int n, Prim* __restrict__ base)
{
    constexpr int kYellow = 0 | (255 << 8) | (255 << 16);
    Prim* __restrict__ top = base + 3 * k;
    Prim* __restrict__ marks = base + 3 * n + 10 * k;
    Prim* __restrict__ bottom = base + 13 * n + 13 * k;

    const double bx1 = row[0], by1 = row[1], bx2 = row[2], by2 = row[3];
    const double of = row[14];
    const bool o_ok = of > -1.0 && of < 4.0;                      // int(of) in 0 .. 3
    const int o = o_ok ? (int)of : -1;
    const bool anchor_ok = coord_ok(bx1) && coord_ok(by1);

    // top picture: box, circle, caption
    if (o_ok && anchor_ok && coord_ok(bx2) && coord_ok(by2)) {
        const int x1 = (int)bx1, y1 = (int)by1, x2 = (int)bx2, y2 = (int)by2;
        const int xa = min(x1, x2), xb = max(x1, x2), ya = min(y1, y2), yb = max(y1, y2);
        const int color = o == 0 ? 0 : o == 1 ? 255 : o == 2 ? (255 << 8) : (255 << 16);
        store_prim(top, make_prim(GPP_DRAW_RECT, 0, xa, ya, xb, yb, color, xa - 1, ya - 1, xb + 1, yb + 1));
    } else store_prim(top, none_prim());
    {
        const double cx = row[4], cy = row[5];
        if (coord_ok(cx) && coord_ok(cy)) {
            const int x = (int)cx, y = (int)cy;
            store_prim(top + 1, make_prim(GPP_DRAW_CIRCLE, 0, x, y, 0, 0, kYellow, x - 4, y - 4, x + 4, y + 4));
        } else store_prim(top + 1, none_prim());
    }
    if (anchor_ok) {
        const int x = (int)bx1, y = (int)by1 - 10;
        store_prim(top + 2, caption_prim(0, x, y, caption_text(row[13], row[12])));
        store_prim(bottom, caption_prim(1, x, y, caption_text(row[13], row[15])));
    } else {
        store_prim(top + 2, none_prim());
        store_prim(bottom, none_prim());
    }

    // markers at the m, r and t keypoints (reference visualization.py:102-104, :116-118)
    {
        const int up_x[3] = {0, -4, 4}, up_y[3] = {-4, 4, 4};
        const int sq_x[4] = {-4, 4, 4, -4}, sq_y[4] = {-4, -4, 4, 4};
        const int dn_x[3] = {0, -4, 4}, dn_y[3] = {4, -4, -4};
        const double mx = row[6], my = row[7], rx = row[8], ry = row[9], tx = row[10], ty = row[11];
        marker<3>(marks, coord_ok(mx) && coord_ok(my), (int)mx, (int)my, up_x, up_y, kYellow);
        marker<4>(marks + 3, coord_ok(rx) && coord_ok(ry), (int)rx, (int)ry, sq_x, sq_y, kYellow);
        marker<3>(marks + 7, coord_ok(tx) && coord_ok(ty), (int)tx, (int)ty, dn_x, dn_y, kYellow);
    }

    // bottom picture: the cuboid's corners R (+-l/2, 0 or -h, +-w/2) + location through P (utils.gpp_utils.cuboid_corners)
    const double h = row[16], w = row[17], l = row[18], lx = row[19], ly = row[20], lz = row[21], r0 = row[22], r1 = row[23], r2 = row[24];
    bool ok = o_ok && isfinite(h) && isfinite(w) && isfinite(l) && isfinite(lx) && isfinite(ly) && isfinite(lz) && isfinite(r0) && isfinite(r1) && isfinite(r2);
    const double theta = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    ok = ok && !(theta > kAngleLimit);
    double R00 = 1.0, R01 = 0.0, R02 = 0.0, R10 = 0.0, R11 = 1.0, R12 = 0.0, R20 = 0.0, R21 = 0.0, R22 = 1.0;
    if (ok && theta > 0.0) {
        const double k0 = r0 / theta, k1 = r1 / theta, k2 = r2 / theta;
        double s, c;
        sincos_small(theta, s, c);
        const double v = 1.0 - c;
        R00 = c + v * k0 * k0;       R01 = v * k0 * k1 - s * k2;  R02 = v * k0 * k2 + s * k1;
        R10 = v * k1 * k0 + s * k2;  R11 = c + v * k1 * k1;       R12 = v * k1 * k2 - s * k0;
        R20 = v * k2 * k0 - s * k1;  R21 = v * k2 * k1 + s * k0;  R22 = c + v * k2 * k2;
    }
    int u[8], v[8];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
        const double xs = (c8 & 2) ? -(l / 2.0) : (l / 2.0);
        const double ys = (c8 & 4) ? -h : 0.0;
        const double zs = ((c8 & 1) ^ ((c8 >> 1) & 1)) ? -(w / 2.0) : (w / 2.0);
        const double X = R00 * xs + R01 * ys + R02 * zs + lx;
        const double Y = R10 * xs + R11 * ys + R12 * zs + ly;
        const double Z = R20 * xs + R21 * ys + R22 * zs + lz;
        const double x0 = P[0] * X + P[1] * Y + P[2] * Z + P[3];
        const double x1 = P[4] * X + P[5] * Y + P[6] * Z + P[7];
        const double x2 = P[8] * X + P[9] * Y + P[10] * Z + P[11];
        const double uu = x0 / x2, vv = x1 / x2;
        ok = ok && (x2 > 0.0) && coord_ok(uu) && coord_ok(vv);
        u[c8] = ok ? (int)uu : 0;
        v[c8] = ok ? (int)vv : 0;
    }
    // the 12 edges in the reference's order (:335-386): the corner pairs are the same for every orientation class, the dashed ones are not
    constexpr int ea[12] = {2, 3, 7, 6, 0, 1, 4, 5, 0, 1, 5, 4}, eb[12] = {3, 7, 6, 2, 3, 2, 7, 6, 1, 5, 4, 0};
    const int dashed = o == 0 ? 0x013 : o == 1 ? 0x029 : o == 2 ? 0x910 : 0x320;       // edges {0,1,4} {0,3,5} {4,8,11} {5,8,9}
    const int color = hsv_color(k, n);
#pragma unroll
    for (int e = 0; e < 12; ++e)
        store_prim(bottom + 1 + e, ok ? line_prim(1, u[ea[e]], v[ea[e]], u[eb[e]], v[eb[e]], color, (dashed >> e) & 1) : none_prim());
}

// exclusive prefix of `flag` over the workgroup's threads and its total; WAVES = threads / 64
template <int WAVES>
__device__ inline int block_scan(bool flag, int* __restrict__ s_wave, int& total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long ballot = __ballot(flag);
    const int before = __popcll(ballot & ((1ull << lane) - 1ull));
    __syncthreads();                                  // (s_wave may still be read from the previous call)
    if (lane == 0) s_wave[wave] = __popcll(ballot);
    __syncthreads();
    int offset = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const int c = s_wave[i];
        if (i < wave) offset += c;
        total += c;
    }
    return offset + before;
}

__global__ __launch_bounds__(kBuildThreads) void draw_build_kernel(const float* __restrict__ rows, const double* __restrict__ P, int D,
                                                                   float score_thr, Prim* __restrict__ prims, int32_t* __restrict__ counts)
{
    __shared__ int s_wave[kBuildThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ rows_b = rows + (size_t)b * D * GPP_POSE_COLS;
    const size_t first = (size_t)b * D * kPerDet;
    // n: the rows with score > threshold (a NaN score is not selected)
    int n = 0;
    for (int d0 = 0; d0 < D; d0 += kBuildThreads) {
        const int d = d0 + tid;
        int total;
        block_scan<kBuildThreads / 64>(d < D && rows_b[(size_t)d * GPP_POSE_COLS + 12] > score_thr, s_wave, total);
        n += total;
    }
    if (tid == 0) {
        counts[4 * b] = n; counts[4 * b + 1] = kPerDet * n; counts[4 * b + 2] = (int32_t)first; counts[4 * b + 3] = 0;
    }
    int running = 0;
    for (int d0 = 0; d0 < D; d0 += kBuildThreads) {
        const int d = d0 + tid;
        const bool sel = d < D && rows_b[(size_t)d * GPP_POSE_COLS + 12] > score_thr;
        int total;
        const int k = running + block_scan<kBuildThreads / 64>(sel, s_wave, total);
        running += total;
        if (sel) build_detection(rows_b + (size_t)d * GPP_POSE_COLS, P + 12 * (size_t)b, k, n, prims + first);
    }
}

// ---------------------------------------------------------------------------------------------- coverage, exact integers
// LINE(p, q): N = max(|dx|, |dy|); for i = 0 .. N the major coordinate is start + i sign, the minor one start + sign(dm) floor((2 i |dm| + N) / (2N))
__device__ inline bool line_covers(long long x0, long long y0, long long x1, long long y1, long long px, long long py)
{
    const long long dx = x1 - x0, dy = y1 - y0;
    const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool x_major = adx >= ady;
    const long long N = x_major ? adx : ady;
    if (N == 0) return px == x0 && py == y0;
    const long long da = x_major ? dx : dy, dm = x_major ? dy : dx, adm = x_major ? ady : adx;
    const long long i = ((x_major ? px - x0 : py - y0)) * (da > 0 ? 1 : -1);
    if (i < 0 || i > N) return false;
    const long long step = (2 * i * adm + N) / (2 * N);
    const long long minor = (x_major ? y0 : x0) + (dm > 0 ? step : dm < 0 ? -step : 0);
    return (x_major ? py : px) == minor;
}

// DASHED(p, q): samples at i = 0, 8, 16, ... < dist, r = i / dist, int(p (1 - r) + q r + .5); LINE(sample j - 1, sample j) for odd j.
// A pixel of dash j lies within three pixels of the real segment between arc lengths 8 (j - 1) and 8 j, so its own arc length / 8,
// rounded down, is j - 2, j - 1 or j: the odd j of [floor - 1, floor + 3] are all that can cover it.
__device__ inline bool dashed_covers(long long x0, long long y0, long long x1, long long y1, long long px, long long py)
{
    const long long dx = x1 - x0, dy = y1 - y0;
    const long long d2 = dx * dx + dy * dy;
    if (d2 == 0) return false;
    const double dist = sqrt((double)d2);
    const long long ns = (long long)ceil(dist / 8.0);                  // samples: 8 j < dist
    if (ns < 2) return false;
    const long long dot = (px - x0) * dx + (py - y0) * dy;
    const long long ju = (long long)floor((double)dot / (dist * 8.0));
    long long j = ju - 1 < 1 ? 1 : ju - 1;
    j |= 1;
    const long long last = ju + 3 < ns - 1 ? ju + 3 : ns - 1;
    for (; j <= last; j += 2) {
        const double ra = (double)(8 * (j - 1)) / dist, rb = (double)(8 * j) / dist;
        const long long ax = (long long)(((double)x0 * (1.0 - ra) + (double)x1 * ra) + .5), ay = (long long)(((double)y0 * (1.0 - ra) + (double)y1 * ra) + .5);
        const long long cx = (long long)(((double)x0 * (1.0 - rb) + (double)x1 * rb) + .5), cy = (long long)(((double)y0 * (1.0 - rb) + (double)y1 * rb) + .5);
        if (line_covers(ax, ay, cx, cy, px, py)) return true;
    }
    return false;
}

__device__ inline bool glyph_pixel(const Prim& q, int len, int cx, int cy)
{
    if (cy < 0 || cy >= 7 || cx < 0) return false;
    const int i = cx / 6, c = cx - 6 * i;
    if (i >= len || c >= 5) return false;
    const uint32_t code = min((q.text[i >> 2] >> (8 * (i & 3))) & 255u, kSpace);
    return (kGlyphs[code] >> (5 * cy + c)) & 1ull;
}

// the colour record q gives pixel (px, py) of its picture, or -1
__device__ inline int covers(const Prim& q, int px, int py)
{
    if (px < q.bx0 || px > q.bx1 || py < q.by0 || py > q.by1) return -1;
    switch (q.kind) {
    case GPP_DRAW_LINE: return line_covers(q.x0, q.y0, q.x1, q.y1, px, py) ? q.color : -1;
    case GPP_DRAW_DASHED: return dashed_covers(q.x0, q.y0, q.x1, q.y1, px, py) ? q.color : -1;
    case GPP_DRAW_RECT: {                                               // thickness 2: the outer box without the inner one
        const long long x = px, y = py;
        const bool outer = x >= (long long)q.x0 - 1 && x <= (long long)q.x1 + 1 && y >= (long long)q.y0 - 1 && y <= (long long)q.y1 + 1;
        const bool inner = x >= (long long)q.x0 + 1 && x <= (long long)q.x1 - 1 && y >= (long long)q.y0 + 1 && y <= (long long)q.y1 - 1;
        return outer && !inner ? q.color : -1;
    }
    case GPP_DRAW_CIRCLE: {                                             // radius 4: 13 <= dx^2 + dy^2 <= 20
        const long long dx = (long long)px - q.x0, dy = (long long)py - q.y0, r2 = dx * dx + dy * dy;
        return r2 >= 13 && r2 <= 20 ? q.color : -1;
    }
    case GPP_DRAW_CAPTION: {                                            // white glyph pixels over their 3 x 3 dilation in black
        const int len = min(max(q.x1, 0), GPP_DRAW_CAPTION_MAX);
        const long long lx = (long long)px - q.x0, ly = (long long)py - ((long long)q.y0 - 6);
        if (lx < -1 || lx > 6 * len || ly < -1 || ly > 7) return -1;
        const int cx = (int)lx, cy = (int)ly;
        if (glyph_pixel(q, len, cx, cy)) return 0xffffff;
        bool near = false;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) near = near || glyph_pixel(q, len, cx + dx, cy + dy);
        return near ? 0 : -1;
    }
    default: return -1;
    }
}

__global__ __launch_bounds__(kRasterThreads) void draw_raster_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ raw_hw,
                                                                     int Hr, int Wr, const Prim* __restrict__ prims,
                                                                     const int32_t* __restrict__ counts, uint8_t* __restrict__ out,
                                                                     int32_t* __restrict__ status)
{
    __shared__ Prim s_list[kChunk];
    __shared__ int s_wave[kRasterThreads / 64];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int h = min(max(raw_hw[2 * b], 0), Hr), w = min(max(raw_hw[2 * b + 1], 0), Wr);
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const bool first_tile = blockIdx.x == 0 && blockIdx.y == 0;          // it also examines every record and reports (status)
    if (!first_tile && (tx0 >= w || ty0 >= 2 * h)) return;
    const int lx = tid & (kTileW - 1), ly = tid / kTileW;
    const int x = tx0 + lx, y = ty0 + ly;
    const bool inside = x < w && y < 2 * h;
    const int pic = y >= h ? 1 : 0, py = y - pic * h;
    const uint8_t* __restrict__ frame_b = frames + (size_t)b * Hr * Wr * 3;
    uint8_t* __restrict__ out_b = out + (size_t)b * 2 * Hr * Wr * 3;
    const int n_prims = max(counts[4 * b + 1], 0);
    const Prim* __restrict__ prims_b = prims + (size_t)max(counts[4 * b + 2], 0);

    int color = -1, rejected = 0;
    bool listed = false;
    for (int hi = n_prims; hi > 0; hi -= kChunk) {                       // chunks of records, the last one first
        const int lo = max(hi - kChunk, 0), idx = lo + tid;
        bool keep = false;
        int4 r0, r1, r2, r3;
        if (idx < hi) {
            const int4* __restrict__ src = reinterpret_cast<const int4*>(prims_b + idx);
            r0 = src[0]; r1 = src[1]; r2 = src[2]; r3 = src[3];
            const int kind = r0.x, picture = r0.y;
            const bool known = kind >= GPP_DRAW_NONE && kind <= GPP_DRAW_CAPTION && (picture == 0 || picture == 1);
            rejected += known ? 0 : 1;
            if (known && kind != GPP_DRAW_NONE) {
                // its bounding box inside its picture, in output rows
                const int bx0 = max(r1.w, 0), bx1 = min(r2.y, w - 1), by0 = max(r2.x, 0), by1 = min(r2.z, h - 1);
                const long long oy0 = (long long)by0 + (long long)picture * h, oy1 = (long long)by1 + (long long)picture * h;
                keep = bx0 <= bx1 && by0 <= by1 && bx1 >= tx0 && bx0 < tx0 + kTileW && oy1 >= ty0 && oy0 < ty0 + kTileH;
            }
        }
        int total;
        const int pos = block_scan<kRasterThreads / 64>(keep, s_wave, total);
        if (keep) {
            int4* __restrict__ dst = reinterpret_cast<int4*>(&s_list[pos]);
            dst[0] = r0; dst[1] = r1; dst[2] = r2; dst[3] = r3;
        }
        __syncthreads();
        if (total > 0) {
            listed = true;
            if (inside && color < 0) {
                for (int i = total - 1; i >= 0; --i) {
                    const Prim& q = s_list[i];
                    if (q.picture != pic) continue;
                    color = covers(q, x, py);
                    if (color >= 0) break;
                }
            }
        }
        // (also the barrier before the next chunk overwrites the list)
        if (__syncthreads_count(inside && color < 0) == 0 && !first_tile) break;
    }

    if (first_tile) {
        // the records of this image that no rule knows (a table not made by gpp_draw_build): counted, never drawn
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) rejected += __shfl_xor(rejected, sft, 64);
        __syncthreads();
        if ((tid & 63) == 0) s_wave[tid >> 6] = rejected;
        __syncthreads();
        if (tid == 0) {
            int bad = 0;
#pragma unroll
            for (int i = 0; i < kRasterThreads / 64; ++i) bad += s_wave[i];
            status[4 * b] = n_prims; status[4 * b + 1] = bad; status[4 * b + 2] = 2 * h; status[4 * b + 3] = w;
        }
    }

    if (!listed) {
        // no record meets this tile: copy, in aligned 32-bit stores (the source bytes are not aligned with them)
        if (y < 2 * h && tx0 < w) {
            const int nb = (min(tx0 + kTileW, w) - tx0) * 3;
            uint8_t* __restrict__ d0 = out_b + ((size_t)y * w + tx0) * 3;
            const uint8_t* __restrict__ s0 = frame_b + ((size_t)py * w + tx0) * 3;
            const int head = min((int)((4u - (unsigned)((uintptr_t)d0 & 3u)) & 3u), nb);
            const int nd = (nb - head) >> 2, tail0 = head + 4 * nd;
            if (lx < nd) {
                const int o = head + 4 * lx;
                const uint32_t v = (uint32_t)s0[o] | ((uint32_t)s0[o + 1] << 8) | ((uint32_t)s0[o + 2] << 16) | ((uint32_t)s0[o + 3] << 24);
                *reinterpret_cast<uint32_t*>(d0 + o) = v;
            } else if (lx >= 48 && lx < 48 + head) {
                d0[lx - 48] = s0[lx - 48];
            } else if (lx >= 52 && lx < 52 + (nb - tail0)) {
                d0[tail0 + lx - 52] = s0[tail0 + lx - 52];
            }
        }
        return;
    }
    if (inside) {
        uint8_t* __restrict__ d = out_b + ((size_t)y * w + x) * 3;
        if (color >= 0) {
            d[0] = (uint8_t)(color & 255); d[1] = (uint8_t)((color >> 8) & 255); d[2] = (uint8_t)((color >> 16) & 255);
        } else {
            const uint8_t* __restrict__ s = frame_b + ((size_t)py * w + x) * 3;
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        }
    }
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// record offsets are int32 (counts): B D 26 must fit (B, D >= 0)
inline bool table_fits(int B, int D)
{
    if (D > INT32_MAX / kPerDet) return false;
    const int64_t per_image = (int64_t)D * kPerDet;
    return per_image == 0 || (int64_t)B <= INT32_MAX / per_image;
}

}  // namespace

extern "C" int gpp_draw_workspace_bytes(int B, int D, size_t* prims_bytes, size_t* workspace_bytes)
{
    if (B < 0 || D < 0 || !prims_bytes || !workspace_bytes) return GPP_ERR_BAD_ARG;
    if (!table_fits(B, D)) return GPP_ERR_BAD_ARG;
    *prims_bytes = (size_t)B * (size_t)D * kPerDet * sizeof(Prim);
    *workspace_bytes = (size_t)B * GPP_DRAW_COUNT_WORDS * sizeof(int32_t);
    return GPP_OK;
}

extern "C" int gpp_draw_build(const float* rows, const double* P, int B, int D, float score_thr, void* prims, int32_t* counts, void* stream)
{
    if (B < 0 || D < 0) return GPP_ERR_BAD_ARG;
    if (B == 0) return GPP_OK;
    if (!P || !counts || (D > 0 && (!rows || !prims))) return GPP_ERR_BAD_ARG;
    if (!aligned(rows, 4) || !aligned(P, 8) || !aligned(prims, 16) || !aligned(counts, 4)) return GPP_ERR_BAD_ARG;
    if (!table_fits(B, D)) return GPP_ERR_BAD_ARG;
    draw_build_kernel<<<dim3((unsigned)B), dim3(kBuildThreads), 0, (hipStream_t)stream>>>(rows, P, D, score_thr, (Prim*)prims, counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_draw_raster(const uint8_t* frames_u8, const int32_t* raw_hw, int Hr, int Wr, const void* prims, const int32_t* counts,
                               int B, uint8_t* out_u8, void* workspace, void* stream)
{
    if (B < 0 || Hr < 0 || Wr < 0) return GPP_ERR_BAD_ARG;
    if (B == 0 || Hr == 0 || Wr == 0) return GPP_OK;
    if (!frames_u8 || !raw_hw || !counts || !out_u8 || !workspace) return GPP_ERR_BAD_ARG;          // (prims may be null: a table of D = 0)
    if (!aligned(raw_hw, 4) || !aligned(prims, 16) || !aligned(counts, 4) || !aligned(workspace, 4)) return GPP_ERR_BAD_ARG;
    const int64_t tiles_x = ((int64_t)Wr + kTileW - 1) / kTileW, tiles_y = (2 * (int64_t)Hr + kTileH - 1) / kTileH;
    if (B > 65535 || tiles_y > 65535 || tiles_x > INT32_MAX) return GPP_ERR_BAD_ARG;
    draw_raster_kernel<<<dim3((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B), dim3(kRasterThreads), 0, (hipStream_t)stream>>>(
        frames_u8, raw_hw, Hr, Wr, (const Prim*)prims, counts, out_u8, (int32_t*)workspace);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
