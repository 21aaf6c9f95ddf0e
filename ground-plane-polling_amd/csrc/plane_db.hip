// Plane-database distillation on gfx950 (MI355X), DESIGN.md section 4.21: from a pool of candidate planes and a labelled dataset, the
// K planes that polling on that dataset loses least with.
//
//   gpp_poll_costs_u16   the (object, plane) cost table: one workgroup per object, planes strided over its 256 lanes, the pair
//                        arithmetic of gpp_poll_f32 (poll_eval.h: the same float32 operations in the same order, this file is built
//                        with -ffp-contract=off and without packed-FP32 instructions like poll.hip), the result a 16-bit key in
//                        polling's own order -- votes first, then the residual sum in 1/1024 m.
//   gpp_plane_select     greedy facility location on that table, exact integers: per pick one many-workgroup launch that adds every
//                        plane's gain and one single-workgroup launch that takes the first arg-max, lowers `best` and clears the gains.
//                        Plain launches in stream order; no cooperative launch, no persistent grid, no spin.
//
//   gpp_pose_costs_u16 / gpp_plane_select_polled   the same two steps for the location error that polling leaves (section 4.23), at the
//                        end of this file: a second table of pose errors (pose_eval.h) and a signed greedy rule.
//
// Nothing of the reference corresponds to this file: the reference ships five fixed databases and no way to make one.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>

#include "gpp.h"
#include "poll_eval.h"
#include "pose_eval.h"

namespace {

constexpr int kThreads = 256;                 // cost and gain kernels: four wavefronts
constexpr int kPickThreads = 1024;            // the pick: one workgroup of sixteen wavefronts
constexpr int kSlabRows = 256;                // rows per workgroup of the gain launch (<= 65 536: the 32-bit partial sums cannot wrap)
constexpr int kGroupsPerBlock = 64;           // 8-plane column groups per workgroup of the gain launch, at most
constexpr unsigned kInvalid = GPP_PLANE_COST_INVALID;

static_assert((int64_t)kSlabRows * 65535 < ((int64_t)1 << 32), "a slab's sum must fit 32 bits");

__global__ void cost_canonical_kernel(const float4* __restrict__ planes, float4* __restrict__ canon, int M)
{
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M) canon[j] = canonical_plane(planes[j]);
}

// the key of one pair (include/gpp.h): polling ranks planes by votes, then by the residual among planes in front of the camera
__device__ __forceinline__ unsigned cost_key(const Hyp& h)
{
    if (h.zc < 0.0f || !(h.res < FLT_MAX)) return kInvalid;       // behind the camera; NaN / inf never win
    float s = h.res * 1024.0f;
    int q = (s < 8191.0f) ? (int)s : 8191;
    return (unsigned)((6 - (int)h.votes) * 8192 + q);
}

__global__ __launch_bounds__(kThreads) void poll_costs_kernel(
    const float* __restrict__ boxes, const float* __restrict__ dims, const int32_t* __restrict__ orient,
    const float* __restrict__ P_inv, const float4* __restrict__ canon, int rows, int D, int M, float thr,
    const int32_t* __restrict__ row_index, uint16_t* __restrict__ table, int64_t pitch, int64_t row_offset)
{
    const int i = blockIdx.x;                                      // one workgroup per listed row
    const int tid = threadIdx.x;
    const int det = row_index ? row_index[i] : i;
    uint16_t* out = table + (row_offset + i) * pitch;
    const bool listed = det >= 0 && det < rows;                    // (a list entry outside the batch reads nothing)
    const int o = listed ? orient[det] : -1;
    if (o < 0) {                                                   // the -1 padding of gpp_label_prep_f64: no plane serves it
        for (int j = tid; j < M; j += kThreads) out[j] = (uint16_t)kInvalid;
        return;
    }
    V3 ray[4];
    poll_rays(boxes + (size_t)det * 12, P_inv + (size_t)(det / D) * 12, ray);
    float target[6];
    poll_targets(dims + (size_t)det * 3, o, target);

    // two planes of a lane per iteration, as poll_kernel<2>: independent divide / square-root chains
    for (int j = tid; j < M; j += 2 * kThreads) {
        const int j1 = j + kThreads;
        Hyp h0 = evaluate(ray, canon[j], target, thr);
        Hyp h1 = evaluate(ray, canon[j1 < M ? j1 : j], target, thr);     // past the end: plane j again, not stored
        out[j] = (uint16_t)cost_key(h0);
        if (j1 < M) out[j1] = (uint16_t)cost_key(h1);
    }
}

// ---------------------------------------------------------------------------------------------------- the selection
__global__ void select_init_kernel(uint16_t* __restrict__ best, int O, unsigned long long* __restrict__ gain, int M,
                                   unsigned long long* __restrict__ trace, int32_t* __restrict__ count, int* __restrict__ done)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < O) best[t] = (uint16_t)kInvalid;
    if (t < M) gain[t] = 0ull;
    if (t == 0) { trace[0] = (unsigned long long)kInvalid * (unsigned long long)O; *count = 0; *done = 0; }
}

// gain[p] += sum over this workgroup's slab of rows of max(0, best[o] - table[o][p]).  A workgroup is GX column groups of 8 planes by
// GY = 256 / GX row phases (GX = 64 unless the table is narrower); a thread reads the 8 planes of a row with one 16-byte load and keeps
// 32-bit partial sums, the workgroup adds them in LDS and one thread per column group adds the slab's sums to the 64-bit gains.
__global__ __launch_bounds__(kThreads) void select_gain_kernel(
    const uint16_t* __restrict__ table, const uint16_t* __restrict__ best, int O, int M, int64_t pitch, int gx_log2,
    unsigned long long* __restrict__ gain, const int* __restrict__ done)
{
    if (*done) return;                                             // (uniform: set by an earlier pick, stream order)
    __shared__ unsigned s_sum[kGroupsPerBlock * 8];
    const int tid = threadIdx.x;
    const int GX = 1 << gx_log2, GY = kThreads >> gx_log2;
    const int tx = tid & (GX - 1), ty = tid >> gx_log2;
    for (int k = tid; k < GX * 8; k += kThreads) s_sum[k] = 0u;
    __syncthreads();
    const int64_t c0 = ((int64_t)blockIdx.y * GX + tx) * 8;        // first plane of this thread's group; c0 + 8 <= pitch when c0 < M
    const int64_t row0 = (int64_t)blockIdx.x * kSlabRows;
    const int64_t row1 = min((int64_t)O, row0 + kSlabRows);
    if (c0 < M) {
        unsigned acc[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        auto add = [&](uint4 v, int b) {
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[2 * k] += (unsigned)max(b - (int)(w[k] & 0xffffu), 0);
                acc[2 * k + 1] += (unsigned)max(b - (int)(w[k] >> 16), 0);
            }
        };
        const uint16_t* col = table + c0;
        int64_t o = row0 + ty;
        for (; o + 3 * GY < row1; o += 4 * GY) {                    // four rows in flight
            uint4 v0 = *(const uint4*)(col + o * pitch);
            uint4 v1 = *(const uint4*)(col + (o + GY) * pitch);
            uint4 v2 = *(const uint4*)(col + (o + 2 * GY) * pitch);
            uint4 v3 = *(const uint4*)(col + (o + 3 * GY) * pitch);
            int b0 = best[o], b1 = best[o + GY], b2 = best[o + 2 * GY], b3 = best[o + 3 * GY];
            add(v0, b0); add(v1, b1); add(v2, b2); add(v3, b3);
        }
        for (; o < row1; o += GY) add(*(const uint4*)(col + o * pitch), (int)best[o]);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (acc[k]) atomicAdd(&s_sum[tx * 8 + k], acc[k]);
    }
    __syncthreads();
    if (ty == 0 && c0 < M) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned v = s_sum[tx * 8 + k];
            if (c0 + k < M && v) atomicAdd(&gain[c0 + k], (unsigned long long)v);      // (pad columns are read, never counted)
        }
    }
}

// pick k: the first index of the largest gain; none left: the done flag.  Then best = min(best, the plane's column), gains cleared.
__global__ __launch_bounds__(kPickThreads) void select_pick_kernel(
    const uint16_t* __restrict__ table, int O, int M, int64_t pitch, int k, int32_t* __restrict__ chosen,
    unsigned long long* __restrict__ trace, uint16_t* __restrict__ best, int32_t* __restrict__ count,
    unsigned long long* __restrict__ gain, int* __restrict__ done)
{
    const int tid = threadIdx.x;
    if (*done) {                                                   // (uniform; this launch never writes the flag before every thread has read it)
        if (tid == 0) { chosen[k] = -1; trace[k + 1] = trace[k]; }
        return;
    }
    unsigned long long g = 0ull;
    int idx = INT_MAX;
    for (int p = tid; p < M; p += kPickThreads) {                  // ascending p: '>' keeps the first maximum
        const unsigned long long v = gain[p];
        if (v > g) { g = v; idx = p; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long og = __shfl_xor(g, s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        if (og > g || (og == g && oi < idx)) { g = og; idx = oi; }
    }
    __shared__ unsigned long long s_g[kPickThreads / 64];
    __shared__ int s_i[kPickThreads / 64];
    if ((tid & 63) == 0) { s_g[tid >> 6] = g; s_i[tid >> 6] = idx; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPickThreads / 64; ++q) {
        const unsigned long long og = s_g[q];
        const int oi = s_i[q];
        if (og > g || (og == g && oi < idx)) { g = og; idx = oi; }
    }
    if (g == 0ull) {                                               // no plane lowers the objective any more
        if (tid == 0) { *done = 1; chosen[k] = -1; trace[k + 1] = trace[k]; }
        return;
    }
    if (tid == 0) { chosen[k] = idx; trace[k + 1] = trace[k] - g; *count = k + 1; }
    for (int o = tid; o < O; o += kPickThreads) {
        const uint16_t t = table[(int64_t)o * pitch + idx];
        if (t < best[o]) best[o] = t;
    }
    for (int p = tid; p < M; p += kPickThreads) gain[p] = 0ull;    // (every gain was read before the barrier above)
}

}  // namespace

extern "C" int gpp_poll_costs_workspace_bytes(int M, size_t* bytes)
{
    if (!bytes || M < 0) return GPP_ERR_BAD_ARG;
    *bytes = sizeof(float) * 4 * (size_t)M;
    return GPP_OK;
}

extern "C" int gpp_poll_costs_u16(const float* boxes, const float* dims, const int32_t* orient, const float* P_inv, const float* planes,
                                  int B, int D, int M, float thr, const int32_t* row_index, int O, uint16_t* table, int64_t pitch,
                                  int64_t row_offset, void* workspace, size_t workspace_bytes, void* stream)
{
    if (B < 0 || D < 0 || M < 0 || O < 0 || row_offset < 0) return GPP_ERR_BAD_ARG;
    if ((int64_t)B * D > INT_MAX) return GPP_ERR_BAD_ARG;
    if (!row_index && O != B * D) return GPP_ERR_BAD_ARG;
    if (pitch < M || pitch % 8 != 0) return GPP_ERR_BAD_ARG;
    if ((int64_t)O * M == 0) return GPP_OK;
    if (!boxes || !dims || !orient || !P_inv || !planes || !table || !workspace) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_ERR_BAD_ARG;                  // a list of rows of an empty batch
    size_t need = 0;
    gpp_poll_costs_workspace_bytes(M, &need);
    if (workspace_bytes < need) return GPP_ERR_WORKSPACE;
    if (((uintptr_t)planes & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)table & 15)) return GPP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    cost_canonical_kernel<<<dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st>>>((const float4*)planes, (float4*)workspace, M);
    poll_costs_kernel<<<dim3((unsigned)O), dim3(kThreads), 0, st>>>(boxes, dims, orient, P_inv, (const float4*)workspace, B * D, D, M, thr,
                                                                    row_index, table, pitch, row_offset);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_plane_select_workspace_bytes(int M, size_t* bytes)
{
    if (!bytes || M < 0) return GPP_ERR_BAD_ARG;
    *bytes = sizeof(unsigned long long) * (size_t)M + 16;          // gain (M), then the done flag
    return GPP_OK;
}

extern "C" int gpp_plane_select(const uint16_t* table, int O, int M, int64_t pitch, int K, int32_t* chosen, uint64_t* trace,
                                uint16_t* best, int32_t* count, void* workspace, size_t workspace_bytes, void* stream)
{
    if (O < 1 || M < 1 || K < 1 || K > M) return GPP_ERR_BAD_ARG;
    if (pitch < M || pitch % 8 != 0) return GPP_ERR_BAD_ARG;
    if (!table || !chosen || !trace || !best || !count || !workspace) return GPP_ERR_BAD_ARG;
    size_t need = 0;
    gpp_plane_select_workspace_bytes(M, &need);
    if (workspace_bytes < need) return GPP_ERR_WORKSPACE;
    if (((uintptr_t)table & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)trace & 7)) return GPP_ERR_ALIGN;
    const int64_t groups = ((int64_t)M + 7) / 8;
    int gx_log2 = 0;
    while ((1 << gx_log2) < kGroupsPerBlock && ((int64_t)1 << gx_log2) < groups) ++gx_log2;
    const int64_t col_blocks = (groups + (1 << gx_log2) - 1) >> gx_log2;
    const int64_t slabs = ((int64_t)O + kSlabRows - 1) / kSlabRows;
    if (col_blocks > 65535) return GPP_ERR_BAD_ARG;                // (M beyond 33 million planes)
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* gain = (unsigned long long*)workspace;
    int* done = (int*)(gain + M);
    const int64_t n = O > M ? O : M;
    select_init_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(best, O, gain, M, (unsigned long long*)trace, count, done);
    for (int k = 0; k < K && hipPeekAtLastError() == hipSuccess; ++k) {     // (a failed launch ends the queueing: the error is returned)
        select_gain_kernel<<<dim3((unsigned)slabs, (unsigned)col_blocks), dim3(kThreads), 0, st>>>(table, best, O, M, pitch, gx_log2, gain, done);
        select_pick_kernel<<<dim3(1), dim3(kPickThreads), 0, st>>>(table, O, M, pitch, k, chosen, (unsigned long long*)trace, best, count, gain, done);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

// ==================================================================================================== the polled location objective
// the same two steps for the location error that polling leaves.  Two tables: keys[o][p] as above, errs[o][p]
// the location error of the pose that plane p alone gives object o (pose_eval.h), in 1/256 m.  The selection follows polling: a row is
// served by the chosen plane of the smallest key (the earlier pick on equal keys), and pays that plane's error.
namespace {

__global__ __launch_bounds__(kThreads) void pose_costs_kernel(
    const float* __restrict__ boxes, const float* __restrict__ dims, const int32_t* __restrict__ orient,
    const float* __restrict__ P_inv, const float* __restrict__ want, const float4* __restrict__ canon, int rows, int D, int M, float thr,
    const int32_t* __restrict__ row_index, uint16_t* __restrict__ keys, uint16_t* __restrict__ errs, int64_t pitch, int64_t row_offset)
{
    const int i = blockIdx.x;                                      // one workgroup per listed row
    const int tid = threadIdx.x;
    const int det = row_index ? row_index[i] : i;
    uint16_t* out_k = keys + (row_offset + i) * pitch;
    uint16_t* out_e = errs + (row_offset + i) * pitch;
    const bool listed = det >= 0 && det < rows;                    // (a list entry outside the batch reads nothing)
    const int o = listed ? orient[det] : -1;
    if (o < 0) {                                                   // the -1 padding of gpp_label_prep_f64: no plane serves it
        for (int j = tid; j < M; j += kThreads) { out_k[j] = (uint16_t)kInvalid; out_e[j] = (uint16_t)kInvalid; }
        return;
    }
    V3 ray[4];
    poll_rays(boxes + (size_t)det * 12, P_inv + (size_t)(det / D) * 12, ray);
    float target[6];
    poll_targets(dims + (size_t)det * 3, o, target);
    const float w = dims[(size_t)det * 3 + 1];
    const V3 goal = {want[(size_t)det * 3], want[(size_t)det * 3 + 1], want[(size_t)det * 3 + 2]};

    // two planes of a lane per iteration, as poll_costs_kernel: independent divide / square-root chains
    for (int j = tid; j < M; j += 2 * kThreads) {
        const int j1 = j + kThreads;
        Hyp h0 = evaluate(ray, canon[j], target, thr);
        Hyp h1 = evaluate(ray, canon[j1 < M ? j1 : j], target, thr);     // past the end: plane j again, not stored
        const unsigned k0 = cost_key(h0), k1 = cost_key(h1);
        const unsigned e0 = pose_error_quanta(h0.X, o, w, goal), e1 = pose_error_quanta(h1.X, o, w, goal);
        out_k[j] = (uint16_t)k0;
        out_e[j] = (uint16_t)(k0 == kInvalid ? kInvalid : e0);
        if (j1 < M) {
            out_k[j1] = (uint16_t)k1;
            out_e[j1] = (uint16_t)(k1 == kInvalid ? kInvalid : e1);
        }
    }
}

static_assert((int64_t)kSlabRows * 65535 < ((int64_t)1 << 24), "a slab's signed sum must fit 32 bits with room to spare");

__global__ void polled_init_kernel(uint16_t* __restrict__ best, uint16_t* __restrict__ cur, int O, unsigned long long* __restrict__ gain,
                                   int M, unsigned long long* __restrict__ trace, int32_t* __restrict__ count, int* __restrict__ done)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < O) { best[t] = (uint16_t)kInvalid; cur[t] = (uint16_t)kInvalid; }
    if (t < M) gain[t] = 0ull;
    if (t == 0) { trace[0] = (unsigned long long)kInvalid * (unsigned long long)O; *count = 0; *done = 0; }
}

// gain[p] += sum over this workgroup's slab of rows with keys[o][p] < best[o] of (cur[o] - errs[o][p]): signed.  The shape of
// select_gain_kernel, with a second 16-byte load per row and signed 32-bit partial sums; the 64-bit gains are two's complement, so the
// unsigned atomic add of a sign-extended slab sum is the signed addition, in any order.
__global__ __launch_bounds__(kThreads) void polled_gain_kernel(
    const uint16_t* __restrict__ keys, const uint16_t* __restrict__ errs, const uint16_t* __restrict__ best,
    const uint16_t* __restrict__ cur, int O, int M, int64_t pitch, int gx_log2, unsigned long long* __restrict__ gain,
    const int* __restrict__ done)
{
    if (*done) return;                                             // (uniform: set by an earlier pick, stream order)
    __shared__ int s_sum[kGroupsPerBlock * 8];
    const int tid = threadIdx.x;
    const int GX = 1 << gx_log2, GY = kThreads >> gx_log2;
    const int tx = tid & (GX - 1), ty = tid >> gx_log2;
    for (int k = tid; k < GX * 8; k += kThreads) s_sum[k] = 0;
    __syncthreads();
    const int64_t c0 = ((int64_t)blockIdx.y * GX + tx) * 8;        // first plane of this thread's group; c0 + 8 <= pitch when c0 < M
    const int64_t row0 = (int64_t)blockIdx.x * kSlabRows;
    const int64_t row1 = min((int64_t)O, row0 + kSlabRows);
    if (c0 < M) {
        int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        auto add = [&](uint4 kv, uint4 ev, int b, int c) {
            const unsigned kw[4] = {kv.x, kv.y, kv.z, kv.w};
            const unsigned ew[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[2 * k] += ((int)(kw[k] & 0xffffu) < b) ? c - (int)(ew[k] & 0xffffu) : 0;
                acc[2 * k + 1] += ((int)(kw[k] >> 16) < b) ? c - (int)(ew[k] >> 16) : 0;
            }
        };
        const uint16_t* kcol = keys + c0;
        const uint16_t* ecol = errs + c0;
        int64_t o = row0 + ty;
        for (; o + GY < row1; o += 2 * GY) {                        // two rows of both tables in flight
            uint4 k0 = *(const uint4*)(kcol + o * pitch);
            uint4 e0 = *(const uint4*)(ecol + o * pitch);
            uint4 k1 = *(const uint4*)(kcol + (o + GY) * pitch);
            uint4 e1 = *(const uint4*)(ecol + (o + GY) * pitch);
            int b0 = best[o], c0_ = cur[o], b1 = best[o + GY], c1 = cur[o + GY];
            add(k0, e0, b0, c0_); add(k1, e1, b1, c1);
        }
        for (; o < row1; o += GY) add(*(const uint4*)(kcol + o * pitch), *(const uint4*)(ecol + o * pitch), (int)best[o], (int)cur[o]);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (acc[k]) atomicAdd(&s_sum[tx * 8 + k], acc[k]);
    }
    __syncthreads();
    if (ty == 0 && c0 < M) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int v = s_sum[tx * 8 + k];
            if (c0 + k < M && v) atomicAdd(&gain[c0 + k], (unsigned long long)(long long)v);     // (pad columns are read, never counted)
        }
    }
}

// pick k: the first index of the largest signed gain; none above 0: the done flag.  Then, along the plane's column, the rows it takes
// over (a strictly smaller key) get its key and its error; gains cleared.
__global__ __launch_bounds__(kPickThreads) void polled_pick_kernel(
    const uint16_t* __restrict__ keys, const uint16_t* __restrict__ errs, int O, int M, int64_t pitch, int k, int32_t* __restrict__ chosen,
    unsigned long long* __restrict__ trace, uint16_t* __restrict__ best, uint16_t* __restrict__ cur, int32_t* __restrict__ count,
    unsigned long long* __restrict__ gain, int* __restrict__ done)
{
    const int tid = threadIdx.x;
    if (*done) {                                                   // (uniform; this launch never writes the flag before every thread has read it)
        if (tid == 0) { chosen[k] = -1; trace[k + 1] = trace[k]; }
        return;
    }
    long long g = 0ll;                                             // (a gain has to be above 0 to be picked)
    int idx = INT_MAX;
    for (int p = tid; p < M; p += kPickThreads) {                  // ascending p: '>' keeps the first maximum
        const long long v = (long long)gain[p];
        if (v > g) { g = v; idx = p; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const long long og = __shfl_xor(g, s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        if (og > g || (og == g && oi < idx)) { g = og; idx = oi; }
    }
    __shared__ long long s_g[kPickThreads / 64];
    __shared__ int s_i[kPickThreads / 64];
    if ((tid & 63) == 0) { s_g[tid >> 6] = g; s_i[tid >> 6] = idx; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kPickThreads / 64; ++q) {
        const long long og = s_g[q];
        const int oi = s_i[q];
        if (og > g || (og == g && oi < idx)) { g = og; idx = oi; }
    }
    if (g <= 0ll) {                                                // no plane lowers the objective any more
        if (tid == 0) { *done = 1; chosen[k] = -1; trace[k + 1] = trace[k]; }
        return;
    }
    if (tid == 0) { chosen[k] = idx; trace[k + 1] = trace[k] - (unsigned long long)g; *count = k + 1; }
    for (int o = tid; o < O; o += kPickThreads) {
        const uint16_t t = keys[(int64_t)o * pitch + idx];
        if (t < best[o]) { best[o] = t; cur[o] = errs[(int64_t)o * pitch + idx]; }
    }
    for (int p = tid; p < M; p += kPickThreads) gain[p] = 0ull;    // (every gain was read before the barrier above)
}

}  // namespace

extern "C" int gpp_pose_costs_u16(const float* boxes, const float* dims, const int32_t* orient, const float* P_inv, const float* want,
                                  const float* planes, int B, int D, int M, float thr, const int32_t* row_index, int O, uint16_t* keys,
                                  uint16_t* errs, int64_t pitch, int64_t row_offset, void* workspace, size_t workspace_bytes, void* stream)
{
    if (B < 0 || D < 0 || M < 0 || O < 0 || row_offset < 0) return GPP_ERR_BAD_ARG;
    if ((int64_t)B * D > INT_MAX) return GPP_ERR_BAD_ARG;
    if (!row_index && O != B * D) return GPP_ERR_BAD_ARG;
    if (pitch < M || pitch % 8 != 0) return GPP_ERR_BAD_ARG;
    if ((int64_t)O * M == 0) return GPP_OK;
    if (!boxes || !dims || !orient || !P_inv || !want || !planes || !keys || !errs || !workspace) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_ERR_BAD_ARG;                  // a list of rows of an empty batch
    size_t need = 0;
    gpp_poll_costs_workspace_bytes(M, &need);
    if (workspace_bytes < need) return GPP_ERR_WORKSPACE;
    if (((uintptr_t)planes & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)keys & 15) || ((uintptr_t)errs & 15)) return GPP_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    cost_canonical_kernel<<<dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st>>>((const float4*)planes, (float4*)workspace, M);
    pose_costs_kernel<<<dim3((unsigned)O), dim3(kThreads), 0, st>>>(boxes, dims, orient, P_inv, want, (const float4*)workspace, B * D, D, M,
                                                                    thr, row_index, keys, errs, pitch, row_offset);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_plane_select_polled_workspace_bytes(int M, size_t* bytes)
{
    if (!bytes || M < 0) return GPP_ERR_BAD_ARG;
    *bytes = sizeof(long long) * (size_t)M + 16;                   // gain (M) int64, then the done flag
    return GPP_OK;
}

extern "C" int gpp_plane_select_polled(const uint16_t* keys, const uint16_t* errs, int O, int M, int64_t pitch, int K, int32_t* chosen,
                                       uint64_t* trace, uint16_t* best, uint16_t* cur, int32_t* count, void* workspace,
                                       size_t workspace_bytes, void* stream)
{
    if (O < 1 || M < 1 || K < 1 || K > M) return GPP_ERR_BAD_ARG;
    if (pitch < M || pitch % 8 != 0) return GPP_ERR_BAD_ARG;
    if (!keys || !errs || !chosen || !trace || !best || !cur || !count || !workspace) return GPP_ERR_BAD_ARG;
    size_t need = 0;
    gpp_plane_select_polled_workspace_bytes(M, &need);
    if (workspace_bytes < need) return GPP_ERR_WORKSPACE;
    if (((uintptr_t)keys & 15) || ((uintptr_t)errs & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)trace & 7)) return GPP_ERR_ALIGN;
    const int64_t groups = ((int64_t)M + 7) / 8;
    int gx_log2 = 0;
    while ((1 << gx_log2) < kGroupsPerBlock && ((int64_t)1 << gx_log2) < groups) ++gx_log2;
    const int64_t col_blocks = (groups + (1 << gx_log2) - 1) >> gx_log2;
    const int64_t slabs = ((int64_t)O + kSlabRows - 1) / kSlabRows;
    if (col_blocks > 65535) return GPP_ERR_BAD_ARG;                // (M beyond 33 million planes)
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* gain = (unsigned long long*)workspace;
    int* done = (int*)(gain + M);
    const int64_t n = O > M ? O : M;
    polled_init_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(best, cur, O, gain, M, (unsigned long long*)trace, count, done);
    for (int k = 0; k < K && hipPeekAtLastError() == hipSuccess; ++k) {     // (a failed launch ends the queueing: the error is returned)
        polled_gain_kernel<<<dim3((unsigned)slabs, (unsigned)col_blocks), dim3(kThreads), 0, st>>>(keys, errs, best, cur, O, M, pitch, gx_log2, gain, done);
        polled_pick_kernel<<<dim3(1), dim3(kPickThreads), 0, st>>>(keys, errs, O, M, pitch, k, chosen, (unsigned long long*)trace, best, cur,
                                                                   count, gain, done);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
