// Per-frame road-plane fit on gfx950 (MI355X), DESIGN.md section 4.22: a consensus fit of one plane to the road region of a LiDAR scan, in
// rectified camera coordinates and in EXACT INTEGERS -- the points are quantised once (256 quanta per metre), every later quantity is an
// integer below 2^53 (carried in int64 or in float64, whichever is cheaper) or a float64 value made by one documented rounded operation, so
// the result does not depend on lane order, atomics order or tile shape.  This file is built with -ffp-contract=off and without packed FP32.
//
//   gpp_road_points_i32   gate and quantise: one workgroup per frame walks its scan in chunks of 256 points, a ballot / LDS scan keeps the
//                         scan's own order (the hypotheses draw points by index)
//   gpp_road_score        count[f][h]: one lane per hypothesis with its plane in registers, slabs of 512 points staged in LDS as float64 and
//                         read as a broadcast, up to 64 workgroups along a frame's points, one atomicAdd of the lane's count per workgroup
//   gpp_road_winner       the largest count, the first hypothesis among equals: the lexicographic reduction of gpp_plane_select's pick
//   gpp_road_moments      ten integer sums over the winner's inliers, 64-bit integer atomics
//   gpp_road_peel_i32     section 4.24, several planes per frame: the kept points that are NOT inliers of the winner, in their order, into a
//                         second buffer -- a stable compaction over many workgroups in three launches (count per block of 2048 points, an
//                         exclusive scan of a frame's block counts, scatter); the next round's score / winner / moments run on the result
//
// Plain launches in stream order; no cooperative launch, no persistent grid, no spin.  The host side -- the 2 x 2 solve on the ten sums -- is
// utils/road_fit.py.  Nothing of the reference corresponds to this file: the reference ships its plane databases and no way to make one.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>

#include "gpp.h"

namespace {

constexpr int kThreads = 256;                 // every kernel here: four wavefronts
constexpr int kSlab = GPP_ROAD_SLAB;          // points per workgroup of the score launch (12 KiB of LDS as float64)
constexpr int kMomentSlab = 2048;             // points per workgroup of the moments launch: 8 per thread
constexpr int kScoreSlabGroups = 64;         // workgroups along a frame's points in the score launch, at most: each walks every 64th slab
constexpr int kPeelBlock = GPP_ROAD_PEEL_BLOCK; // points per workgroup of the peel's count and scatter launches: 8 chunks of 256
constexpr int kMaxFrames = 65535;             // frames are the grid's z (score) or y (moments) dimension

__device__ __forceinline__ uint32_t mix(uint32_t u)
{
    u ^= u >> 16; u *= 0x7feb352du; u ^= u >> 15; u *= 0x846ca68bu; u ^= u >> 16;
    return u;
}

// the frame's segment [base, base + n) of the ragged batch; offsets that leave [0, total], descend or exceed max_points: an empty frame
__device__ __forceinline__ void frame_segment(const int32_t* __restrict__ offsets, int f, int total, int max_points, int64_t& base, int& n)
{
    const int a = offsets[f], b = offsets[f + 1];
    const bool ok = a >= 0 && b >= a && b <= total && b - a <= max_points;
    base = ok ? a : 0;
    n = ok ? b - a : 0;
}

__device__ __forceinline__ int frame_kept(const int32_t* __restrict__ kept, int f, int n)
{
    const int m = kept[f];
    return m < 0 ? 0 : (m > n ? n : m);
}

struct Plane { double nx, ny, nz, d0, nn; bool valid; };

// hypothesis h of a frame of m kept points at q: three draws, n = (p1 - p0) x (p2 - p0) and d0 = n . p0 in int64 (|n| < 2^33, |d0| < 2^51:
// gpp.h), then the gates on float64 -- nn, the products with c2 / hlo2 / hhi2 and the squares are single rounded operations
__device__ __forceinline__ Plane road_plane(const int32_t* __restrict__ q, int m, uint32_t key, uint32_t h, double c2, double hlo2, double hhi2)
{
    Plane P;
    P.nx = P.ny = P.nz = P.d0 = P.nn = 0.0;
    P.valid = false;
    if (m < 3) return P;
    const uint32_t kh = mix(key + h);
    int64_t p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t i = __umulhi(mix(kh + (uint32_t)k), (uint32_t)m);        // (uint64(r) * m) >> 32  <  m
        const int32_t* s = q + (int64_t)i * 3;
        p[k][0] = s[0]; p[k][1] = s[1]; p[k][2] = s[2];
    }
    const int64_t ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const int64_t bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const int64_t nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const int64_t d0 = nx * p[0][0] + ny * p[0][1] + nz * p[0][2];
    P.nx = (double)nx; P.ny = (double)ny; P.nz = (double)nz; P.d0 = (double)d0;
    P.nn = (P.nx * P.nx + P.ny * P.ny) + P.nz * P.nz;
    const double dd = P.d0 * P.d0;
    P.valid = P.nn > 0.0 && P.ny * P.ny >= c2 * P.nn && hlo2 * P.nn <= dd && dd <= hhi2 * P.nn;
    return P;
}

// ---------------------------------------------------------------------------------------------------- gate and quantise
__global__ __launch_bounds__(kThreads) void road_points_kernel(
    const float4* __restrict__ points, const int32_t* __restrict__ offsets, const double* __restrict__ T, int total, int max_points,
    double xq, double yq, double zq, int32_t* __restrict__ q, int32_t* __restrict__ kept)
{
    __shared__ int s_wave[kThreads / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t base;
    int n;
    frame_segment(offsets, f, total, max_points, base, n);
    double t[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) t[k] = T[(int64_t)f * 12 + k];
    int32_t* out = q + base * 3;
    int written = 0;                                               // (uniform: every thread adds the same chunk totals)
    for (int at = 0; at < n; at += kThreads) {
        const int i = at + tid;
        bool keep = false;
        double v[3] = {0.0, 0.0, 0.0};
        if (i < n) {
            const float4 pt = points[base + i];
            const double x = pt.x, y = pt.y, z = pt.z;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                v[r] = floor((((t[4 * r] * x + t[4 * r + 1] * y) + t[4 * r + 2] * z) + t[4 * r + 3]) * 256.0 + 0.5);
            keep = fabs(v[0]) <= xq && fabs(v[1]) <= yq && v[2] >= 1.0 && v[2] <= zq;      // NaN and infinity fail
        }
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int prefix = written, sum = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int c = s_wave[w];
            if (w < wave) prefix += c;
            sum += c;
        }
        if (keep) {
            int32_t* o = out + (int64_t)(prefix + before) * 3;      // prefix + before < n: inside the frame's own segment
            o[0] = (int32_t)v[0]; o[1] = (int32_t)v[1]; o[2] = (int32_t)v[2];
        }
        written += sum;
        __syncthreads();                                           // (s_wave is rewritten by the next chunk)
    }
    if (tid == 0) kept[f] = written;
}

// ---------------------------------------------------------------------------------------------------- score
__global__ __launch_bounds__(kThreads) void road_score_kernel(
    const int32_t* __restrict__ q, const int32_t* __restrict__ offsets, const int32_t* __restrict__ kept,
    const uint32_t* __restrict__ frame_id, uint32_t seed, int H, int total, int max_points,
    double c2, double hlo2, double hhi2, double tq2, int32_t* __restrict__ count)
{
    __shared__ double s_p[kSlab * 3];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int h = blockIdx.x * kThreads + tid;
    int64_t base;
    int n;
    frame_segment(offsets, f, total, max_points, base, n);
    const int m = frame_kept(kept, f, n);
    if (blockIdx.y > 0 && (int)blockIdx.y * kSlab >= m) return;    // (uniform) no slab of this frame for this workgroup; y = 0 still marks the invalid
    const int32_t* qf = q + base * 3;
    Plane P = {0.0, 0.0, 0.0, 0.0, 0.0, false};
    if (h < H) P = road_plane(qf, m, mix(seed + frame_id[f]), (uint32_t)h, c2, hlo2, hhi2);
    const double t2 = P.valid ? tq2 * P.nn : -1.0, nd0 = -P.d0;    // (an invalid lane counts nothing: dot dot >= 0 > -1)
    int c = 0;
    for (int p0 = (int)blockIdx.y * kSlab; p0 < m; p0 += (int)gridDim.y * kSlab) {      // (uniform) this workgroup's slabs
        const int cnt = min(kSlab, m - p0);
        __syncthreads();                                           // (the slab before has been read)
        for (int k = tid; k < cnt * 3; k += kThreads) s_p[k] = (double)qf[(int64_t)p0 * 3 + k];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            // n . p - d0: integers below 2^51 at every step, so the fused form is exact like the separate one
            const double dot = fma(P.nx, s_p[3 * j], fma(P.ny, s_p[3 * j + 1], fma(P.nz, s_p[3 * j + 2], nd0)));
            c += (dot * dot <= t2) ? 1 : 0;
        }
    }
    if (h >= H) return;
    int32_t* out = count + (int64_t)f * H + h;
    if (!P.valid) {
        if (blockIdx.y == 0) *out = -1;                            // (no workgroup adds to an invalid hypothesis: every one finds it invalid)
        return;
    }
    if (c) atomicAdd(out, c);
}

// ---------------------------------------------------------------------------------------------------- winner
__global__ __launch_bounds__(kThreads) void road_winner_kernel(const int32_t* __restrict__ count, int H, int min_inliers,
                                                               int32_t* __restrict__ winner, int32_t* __restrict__ inliers)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    int g = -1, idx = INT_MAX;
    for (int h = tid; h < H; h += kThreads) {                      // ascending h: '>' keeps the first maximum
        const int v = count[(int64_t)f * H + h];
        if (v > g) { g = v; idx = h; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int og = __shfl_xor(g, s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        if (og > g || (og == g && oi < idx)) { g = og; idx = oi; }
    }
    __shared__ int s_g[kThreads / 64];
    __shared__ int s_i[kThreads / 64];
    if ((tid & 63) == 0) { s_g[tid >> 6] = g; s_i[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int og = s_g[w], oi = s_i[w];
            if (og > g || (og == g && oi < idx)) { g = og; idx = oi; }
        }
        winner[f] = (g >= 0 && g >= min_inliers) ? idx : -1;
        inliers[f] = g > 0 ? g : 0;
    }
}

// ---------------------------------------------------------------------------------------------------- moments
__global__ __launch_bounds__(kThreads) void road_moments_kernel(
    const int32_t* __restrict__ q, const int32_t* __restrict__ offsets, const int32_t* __restrict__ kept,
    const uint32_t* __restrict__ frame_id, uint32_t seed, const int32_t* __restrict__ winner, int H, int total, int max_points,
    double tq2, unsigned long long* __restrict__ sums)
{
    __shared__ long long s_sum[kThreads / 64][10];
    const int f = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    const int w = winner[f];
    if (w < 0 || w >= H) return;                                   // (uniform) an invalid frame keeps its zero sums
    int64_t base;
    int n;
    frame_segment(offsets, f, total, max_points, base, n);
    const int m = frame_kept(kept, f, n);
    const int p0 = slab * kMomentSlab;
    if (p0 >= m) return;
    const int32_t* qf = q + base * 3;
    // the winner's plane from its three draws; the gates held when it was scored (c2 = 0, hlo2 = 0, hhi2 = inf: only nn > 0 is asked here)
    const Plane P = road_plane(qf, m, mix(seed + frame_id[f]), (uint32_t)w, 0.0, 0.0, __builtin_huge_val());
    if (!P.valid) return;
    const double t2 = tq2 * P.nn, nd0 = -P.d0;
    long long a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int p1 = min(m, p0 + kMomentSlab);
    for (int i = p0 + tid; i < p1; i += kThreads) {
        const int32_t* s = qf + (int64_t)i * 3;
        const int xi = s[0], yi = s[1], zi = s[2];
        const long long x = xi, y = yi, z = zi;
        const double dot = fma(P.nx, (double)xi, fma(P.ny, (double)yi, fma(P.nz, (double)zi, nd0)));
        if (dot * dot <= t2) {
            a[0] += 1; a[1] += x; a[2] += y; a[3] += z;
            a[4] += x * x; a[5] += x * z; a[6] += z * z; a[7] += x * y; a[8] += z * y; a[9] += y * y;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        long long v = a[k];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
        if ((tid & 63) == 0) s_sum[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < 10) {
        long long v = 0;
#pragma unroll
        for (int wv = 0; wv < kThreads / 64; ++wv) v += s_sum[wv][tid];
        if (v) atomicAdd(&sums[(int64_t)f * 10 + tid], (unsigned long long)v);      // (two's complement: the wrapped sum is the signed sum)
    }
}

// ---------------------------------------------------------------------------------------------------- peel (section 4.24)
// What the three peel launches know of a frame: its segment, its kept points and the winner's plane, recomputed from the three draws as
// gpp_road_moments does (only nn > 0 is asked).  live: the frame has a winner in [0, H); a frame without one is finished (no survivor).
// A winner whose plane has nn = 0 (hand-set only: such a hypothesis is never scored) has no inliers, as in gpp_road_moments.
struct PeelFrame { const int32_t* qf; int64_t base; int m; bool live; double nx, ny, nz, nd0, t2; };

__device__ __forceinline__ PeelFrame peel_frame(const int32_t* __restrict__ q, const int32_t* __restrict__ offsets,
                                                const int32_t* __restrict__ kept, const uint32_t* __restrict__ frame_id, uint32_t seed,
                                                const int32_t* __restrict__ winner, int f, int H, int total, int max_points, double tq2)
{
    PeelFrame R;
    int n;
    frame_segment(offsets, f, total, max_points, R.base, n);
    R.m = frame_kept(kept, f, n);
    R.qf = q + R.base * 3;
    const int w = winner[f];
    R.live = w >= 0 && w < H;
    R.nx = R.ny = R.nz = R.nd0 = 0.0;
    R.t2 = -1.0;                                                   // (no inlier: dot dot >= 0 > -1)
    if (R.live && R.m > 0) {
        const Plane P = road_plane(R.qf, R.m, mix(seed + frame_id[f]), (uint32_t)w, 0.0, 0.0, __builtin_huge_val());
        if (P.valid) { R.nx = P.nx; R.ny = P.ny; R.nz = P.nz; R.nd0 = -P.d0; R.t2 = tq2 * P.nn; }
    }
    return R;
}

// point i of the frame survives the round: it is no inlier of the winner (the test of gpp_road_moments, operation for operation)
__device__ __forceinline__ bool peel_survives(const PeelFrame& R, int i, int& xi, int& yi, int& zi)
{
    const int32_t* s = R.qf + (int64_t)i * 3;
    xi = s[0]; yi = s[1]; zi = s[2];
    const double dot = fma(R.nx, (double)xi, fma(R.ny, (double)yi, fma(R.nz, (double)zi, R.nd0)));
    return !(dot * dot <= R.t2);
}

// (a) block_count[f][b]: the survivors among the frame's kept points [b 2048, b 2048 + 2048); every workgroup writes its word
__global__ __launch_bounds__(kThreads) void road_peel_count_kernel(
    const int32_t* __restrict__ q, const int32_t* __restrict__ offsets, const int32_t* __restrict__ kept,
    const uint32_t* __restrict__ frame_id, uint32_t seed, const int32_t* __restrict__ winner, int H, int total, int max_points,
    double tq2, int32_t* __restrict__ block_count)
{
    __shared__ int s_wave[kThreads / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    int32_t* out = block_count + (int64_t)f * gridDim.x + blockIdx.x;
    const PeelFrame R = peel_frame(q, offsets, kept, frame_id, seed, winner, f, H, total, max_points, tq2);
    const int p0 = (int)blockIdx.x * kPeelBlock;
    if (!R.live || p0 >= R.m) {                                    // (uniform)
        if (tid == 0) *out = 0;
        return;
    }
    const int p1 = min(R.m, p0 + kPeelBlock);
    int c = 0;
    for (int i = p0 + tid; i < p1; i += kThreads) {
        int xi, yi, zi;
        c += peel_survives(R, i, xi, yi, zi) ? 1 : 0;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
    if ((tid & 63) == 0) s_wave[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) v += s_wave[w];
        *out = v;
    }
}

// (b) one workgroup per frame: block_count[f][0 .. blocks) becomes its own exclusive scan, kept_out[f] the total.  Up to 512 blocks: the
// workgroup walks them in chunks of 256 with a running carry
__global__ __launch_bounds__(kThreads) void road_peel_scan_kernel(int32_t* __restrict__ block_count, int blocks, int32_t* __restrict__ kept_out)
{
    __shared__ int s_wave[kThreads / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* row = block_count + (int64_t)f * blocks;
    int carry = 0;                                                 // (uniform)
    for (int at = 0; at < blocks; at += kThreads) {
        const int b = at + tid;
        const int v = b < blocks ? row[b] : 0;
        int incl = v;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int o = __shfl_up(incl, s, 64);
            if (lane >= s) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int prefix = carry, sum = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int c = s_wave[w];
            if (w < wave) prefix += c;
            sum += c;
        }
        if (b < blocks) row[b] = prefix + incl - v;
        carry += sum;
        __syncthreads();                                           // (s_wave is rewritten by the next chunk)
    }
    if (tid == 0) kept_out[f] = carry;
}

// (c) the grid of (a): the mask again, every survivor to q_out at the block's scanned start + its rank inside the block -- chunks of 256
// points, a ballot per wavefront and an LDS prefix across the four, as in road_points_kernel: the order is kept
__global__ __launch_bounds__(kThreads) void road_peel_scatter_kernel(
    const int32_t* __restrict__ q, const int32_t* __restrict__ offsets, const int32_t* __restrict__ kept,
    const uint32_t* __restrict__ frame_id, uint32_t seed, const int32_t* __restrict__ winner, int H, int total, int max_points,
    double tq2, const int32_t* __restrict__ block_start, int32_t* __restrict__ q_out)
{
    __shared__ int s_wave[kThreads / 64];
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PeelFrame R = peel_frame(q, offsets, kept, frame_id, seed, winner, f, H, total, max_points, tq2);
    const int p0 = (int)blockIdx.x * kPeelBlock;
    if (!R.live || p0 >= R.m) return;                              // (uniform)
    const int p1 = min(R.m, p0 + kPeelBlock);
    int32_t* out = q_out + R.base * 3;
    int written = block_start[(int64_t)f * gridDim.x + blockIdx.x];      // (uniform) survivors of the frame before this block: <= p0
    for (int at = p0; at < p1; at += kThreads) {
        const int i = at + tid;
        int xi = 0, yi = 0, zi = 0;
        const bool keep = i < p1 && peel_survives(R, i, xi, yi, zi);
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int prefix = written, sum = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int c = s_wave[w];
            if (w < wave) prefix += c;
            sum += c;
        }
        if (keep) {
            int32_t* o = out + (int64_t)(prefix + before) * 3;      // prefix + before <= i < m: inside the frame's own segment
            o[0] = xi; o[1] = yi; o[2] = zi;
        }
        written += sum;
        __syncthreads();                                           // (s_wave is rewritten by the next chunk)
    }
}

bool ragged_ok(int F, int total, int max_points)
{
    return F >= 0 && F <= kMaxFrames && total >= 0 && total <= GPP_ROAD_MAX_TOTAL && max_points >= 0 && max_points <= GPP_ROAD_MAX_POINTS &&
           max_points <= total;
}

}  // namespace

extern "C" int gpp_road_points_i32(const float* points, const int32_t* offsets, const double* T, int F, int total, int max_points,
                                   int xq, int yq, int zq, int32_t* q, int32_t* kept, void* stream)
{
    if (!ragged_ok(F, total, max_points)) return GPP_ERR_BAD_ARG;
    if (xq < 0 || yq < 0 || zq < 1 || xq > GPP_ROAD_MAX_XQ || yq > GPP_ROAD_MAX_YQ || zq > GPP_ROAD_MAX_ZQ) return GPP_ERR_BAD_ARG;
    if (F == 0) return GPP_OK;
    if (!offsets || !T || !kept || (total > 0 && (!points || !q))) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)points & 15) || ((uintptr_t)T & 7)) return GPP_ERR_ALIGN;
    road_points_kernel<<<dim3((unsigned)F), dim3(kThreads), 0, (hipStream_t)stream>>>(
        (const float4*)points, offsets, T, total, max_points, (double)xq, (double)yq, (double)zq, q, kept);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_road_score(const int32_t* q, const int32_t* offsets, const int32_t* kept, const uint32_t* frame_id, uint32_t seed,
                              int F, int total, int max_points, int H, double c2, double hlo2, double hhi2, double tq2,
                              int32_t* count, void* stream)
{
    if (!ragged_ok(F, total, max_points) || H < 0 || H > GPP_ROAD_MAX_HYPOTHESES) return GPP_ERR_BAD_ARG;
    if (!(c2 >= 0.0 && c2 <= 1.0) || !(hlo2 >= 0.0) || !(hhi2 >= hlo2) || !(tq2 >= 0.0)) return GPP_ERR_BAD_ARG;      // (a NaN fails every one)
    if (F == 0 || H == 0) return GPP_OK;
    if (!offsets || !kept || !frame_id || !count || (total > 0 && !q)) return GPP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)F * (size_t)H, st);
    if (e != hipSuccess) return (int)e;
    int slabs = (max_points + kSlab - 1) / kSlab;
    slabs = slabs < 1 ? 1 : (slabs > kScoreSlabGroups ? kScoreSlabGroups : slabs);
    road_score_kernel<<<dim3((unsigned)((H + kThreads - 1) / kThreads), (unsigned)slabs, (unsigned)F), dim3(kThreads), 0, st>>>(
        q, offsets, kept, frame_id, seed, H, total, max_points, c2, hlo2, hhi2, tq2, count);
    e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_road_winner(const int32_t* count, int F, int H, int min_inliers, int32_t* winner, int32_t* inliers, void* stream)
{
    if (F < 0 || F > kMaxFrames || H < 0 || H > GPP_ROAD_MAX_HYPOTHESES || min_inliers < 1) return GPP_ERR_BAD_ARG;
    if (F == 0) return GPP_OK;
    if (!winner || !inliers || (H > 0 && !count)) return GPP_ERR_BAD_ARG;
    road_winner_kernel<<<dim3((unsigned)F), dim3(kThreads), 0, (hipStream_t)stream>>>(count, H, min_inliers, winner, inliers);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_road_moments(const int32_t* q, const int32_t* offsets, const int32_t* kept, const uint32_t* frame_id, uint32_t seed,
                                const int32_t* winner, int F, int total, int max_points, int H, double tq2, int64_t* sums, void* stream)
{
    if (!ragged_ok(F, total, max_points) || H < 0 || H > GPP_ROAD_MAX_HYPOTHESES || !(tq2 >= 0.0)) return GPP_ERR_BAD_ARG;
    if (F == 0) return GPP_OK;
    if (!offsets || !kept || !frame_id || !winner || !sums || (total > 0 && !q)) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)sums & 7) return GPP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(int64_t) * 10 * (size_t)F, st);
    if (e != hipSuccess) return (int)e;
    const unsigned slabs = (unsigned)((max_points + kMomentSlab - 1) / kMomentSlab);
    if (slabs == 0 || H == 0) return GPP_OK;
    road_moments_kernel<<<dim3(slabs, (unsigned)F), dim3(kThreads), 0, st>>>(
        q, offsets, kept, frame_id, seed, winner, H, total, max_points, tq2, (unsigned long long*)sums);
    e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_road_peel_workspace_bytes(int F, int max_points, size_t* bytes)
{
    if (!bytes || F < 0 || F > kMaxFrames || max_points < 0 || max_points > GPP_ROAD_MAX_POINTS) return GPP_ERR_BAD_ARG;
    const size_t blocks = ((size_t)max_points + kPeelBlock - 1) / kPeelBlock;
    *bytes = sizeof(int32_t) * (size_t)F * blocks + 16;            // a frame's block counts, then their scan in place; never zero
    return GPP_OK;
}

extern "C" int gpp_road_peel_i32(const int32_t* q_in, const int32_t* offsets, const int32_t* kept_in, const uint32_t* frame_id, uint32_t seed,
                                 const int32_t* winner, int F, int total, int max_points, int H, double tq2,
                                 int32_t* q_out, int32_t* kept_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!ragged_ok(F, total, max_points) || H < 0 || H > GPP_ROAD_MAX_HYPOTHESES || !(tq2 >= 0.0)) return GPP_ERR_BAD_ARG;
    if (F == 0) return GPP_OK;
    if (!offsets || !kept_in || !frame_id || !winner || !kept_out || !workspace || (total > 0 && (!q_in || !q_out))) return GPP_ERR_BAD_ARG;
    if (total > 0) {                                               // the two point buffers are distinct: a survivor may land on a row not yet read
        const uintptr_t a = (uintptr_t)q_in, b = (uintptr_t)q_out, span = sizeof(int32_t) * 3 * (uintptr_t)total;
        if (a < b ? b - a < span : a - b < span) return GPP_ERR_BAD_ARG;
    }
    size_t need = 0;
    gpp_road_peel_workspace_bytes(F, max_points, &need);
    if (workspace_bytes < need) return GPP_ERR_WORKSPACE;
    if (((uintptr_t)q_in & 3) || ((uintptr_t)q_out & 3) || ((uintptr_t)kept_out & 3) || ((uintptr_t)workspace & 3)) return GPP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((max_points + kPeelBlock - 1) / kPeelBlock);
    int32_t* block_count = (int32_t*)workspace;
    if (blocks > 0)
        road_peel_count_kernel<<<dim3(blocks, (unsigned)F), dim3(kThreads), 0, st>>>(
            q_in, offsets, kept_in, frame_id, seed, winner, H, total, max_points, tq2, block_count);
    road_peel_scan_kernel<<<dim3((unsigned)F), dim3(kThreads), 0, st>>>(block_count, (int)blocks, kept_out);
    if (blocks > 0)
        road_peel_scatter_kernel<<<dim3(blocks, (unsigned)F), dim3(kThreads), 0, st>>>(
            q_in, offsets, kept_in, frame_id, seed, winner, H, total, max_points, tq2, block_count, q_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
