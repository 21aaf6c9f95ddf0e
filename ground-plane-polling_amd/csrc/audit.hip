// Range audit of dtype='f16x3' (DESIGN.md section 4.12): the largest |x| of every channel of one NHWC map, as the three forms an x3
// convolution reads its activation operand in: plain float32 rows, or pre-split rows whose every 32 channels are
// 128 bytes [32 halves hi | 32 halves lo] (IEEE half or bf16), value = float(hi) + float(lo).
//   out[c] = max(out[c], bits(|x[m, c]|)) over the M pixels: non-negative floats order like their bit patterns, so the maximum is an
//   INTEGER maximum -- independent of the order of arrival, a NaN (bits above 0x7f800000) wins and stays visible, and a launch adds to
//   what earlier launches left in the table (two half batches, five pyramid levels).  The caller clears the table.
// A bandwidth kernel: 16-byte loads per lane, lanes along the channel axis (a wavefront reads whole rows / whole 128-byte channel groups of
// consecutive pixels), running maxima in registers over a grid-stride loop with several rows in flight per lane, the rows of a workgroup
// combined through LDS, then one relaxed agent-scope atomic max per channel per workgroup, issued as runs of consecutive words.  Every
// workgroup of a launch updates the same C words, and such contended atomics are what the first form of this kernel spent its time on
// (1024 workgroups x C atomics per launch: 28 ms against 10 ms for the B = 8 step, profiles/range_audit): a workgroup therefore takes at
// least kMinRows rows per lane, so that a launch issues at most one atomic per kMinRows x 16 bytes it reads.  No floating-point
// arithmetic in the float32 form; one exact conversion pair and one add per value in the split forms.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpp.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;        // 4 workgroups of 4 wavefronts per CU on 256 CUs
constexpr int kMinRows = 64;            // rows per lane before a map is spread over one more workgroup
constexpr uint32_t kAbs = 0x7fffffffu;

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__device__ __forceinline__ float half_value(uint32_t h16, bool bf16)
{
    if (bf16) return __uint_as_float(h16 << 16);
    const _Float16 h = __builtin_bit_cast(_Float16, (uint16_t)h16);
    return (float)h;
}

// One column = one 16-byte unit of float32 (4 channels, N = 4) or one (hi, lo) pair of 16-byte units of a split row (8 channels, N = 8).
// VEC = false: one float32 channel per column (rows that are not 16-byte aligned, C not a multiple of 4).
template <int N, bool VEC, bool BF16>
struct Column {
    uint32_t m[N];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < N; ++k) m[k] = 0;
    }
    // p: the row's first audited channel; col: the column inside the row
    __device__ __forceinline__ void take(const float* p, int col)
    {
        if constexpr (N == 1) {
            m[0] = umax(m[0], __float_as_uint(p[col]) & kAbs);
        } else if constexpr (N == 4) {
            const u32x4 v = *(const u32x4*)(p + col * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = umax(m[k], v[k] & kAbs);
        } else {
            // chunk = 32 channels = 32 float32-sized elements; unit u of the chunk's hi half, the same unit of its lo half 64 bytes on
            const float* q = p + (col >> 2) * 32 + (col & 3) * 4;
            const u32x4 hi = *(const u32x4*)q, lo = *(const u32x4*)(q + 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = half_value(hi[k] & 0xffffu, BF16) + half_value(lo[k] & 0xffffu, BF16);
                const float b = half_value(hi[k] >> 16, BF16) + half_value(lo[k] >> 16, BF16);
                m[2 * k] = umax(m[2 * k], __float_as_uint(a) & kAbs);
                m[2 * k + 1] = umax(m[2 * k + 1], __float_as_uint(b) & kAbs);
            }
        }
    }
    __device__ __forceinline__ void merge(const Column& o)
    {
#pragma unroll
        for (int k = 0; k < N; ++k) m[k] = umax(m[k], o.m[k]);
    }
};

// grid (row blocks, column chunks of up to 256 columns); a workgroup walks rows_par rows at a time
template <int N, bool VEC, bool BF16>
__global__ __launch_bounds__(kThreads) void channel_absmax_kernel(const float* __restrict__ base, int64_t M, int64_t pitch, int cols,
                                                                   uint32_t* __restrict__ out)
{
    __shared__ uint32_t part[kThreads * N];
    const int col0 = blockIdx.y * kThreads;
    const int ncol = min(cols - col0, kThreads);            // columns of this chunk
    const int rows_par = kThreads / ncol;
    const int t = threadIdx.x;
    const int r = t / ncol, col = col0 + t % ncol;
    Column<N, VEC, BF16> acc;
    acc.clear();
    if (r < rows_par) {
        const int64_t step = (int64_t)gridDim.x * rows_par;
        int64_t m = (int64_t)blockIdx.x * rows_par + r;
        constexpr int U = N == 8 ? 4 : 8;                   // independent rows in flight per lane (128 bytes of loads either way)
        for (; m + (U - 1) * step < M; m += U * step) {
            Column<N, VEC, BF16> a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) a[u].clear(), a[u].take(base + (m + u * step) * pitch, col);
#pragma unroll
            for (int u = 0; u < U; ++u) acc.merge(a[u]);
        }
        for (; m < M; m += step) acc.take(base + m * pitch, col);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) part[k * kThreads + t] = acc.m[k];
    __syncthreads();
    if (r == 0)
        for (int q = 1; q < rows_par; ++q)
#pragma unroll
            for (int k = 0; k < N; ++k) acc.m[k] = umax(acc.m[k], part[k * kThreads + q * ncol + t]);
    __syncthreads();
    if (r == 0) {
        // in channel order: value k of a column is channel N col + k; or, split: unit u of chunk c holds channels 32 c + 8 u + k
        const int c = N == 8 ? (t >> 2) * 32 + (t & 3) * 8 : t * N;
#pragma unroll
        for (int k = 0; k < N; ++k) part[c + k] = acc.m[k];
    }
    __syncthreads();
    // consecutive lanes, consecutive words: an atomic instruction of a wavefront covers 256 contiguous bytes
    for (int c = t; c < ncol * N; c += kThreads)
        if (part[c]) __hip_atomic_fetch_max(out + col0 * N + c, part[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int N, bool VEC, bool BF16>
int launch(const float* base, int64_t M, int64_t pitch, int cols, uint32_t* out, void* stream)
{
    const int chunks = (cols + kThreads - 1) / kThreads;
    const int rows_par = kThreads / (cols < kThreads ? cols : kThreads);
    int64_t blocks = (M + (int64_t)rows_par * kMinRows - 1) / ((int64_t)rows_par * kMinRows);
    const int64_t cap = kMaxBlocks / chunks > 0 ? kMaxBlocks / chunks : 1;
    if (blocks > cap) blocks = cap;
    channel_absmax_kernel<N, VEC, BF16><<<dim3((unsigned)blocks, (unsigned)chunks), kThreads, 0, (hipStream_t)stream>>>(base, M, pitch, cols, out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int gpp_channel_absmax(const gpp_absmax_desc* d, void* stream)
{
    if (!d || !d->in || !d->out) return GPP_ERR_BAD_ARG;
    if (d->M < 0 || d->C <= 0 || d->pitch < d->C || d->c_off < 0 || d->c_off + (int64_t)d->C > d->pitch || d->reserved != 0) return GPP_ERR_BAD_ARG;
    if (d->layout != GPP_ABSMAX_F32 && d->layout != GPP_ABSMAX_SPLIT_F16 && d->layout != GPP_ABSMAX_SPLIT_BF16) return GPP_ERR_BAD_ARG;
    if (d->M * d->pitch >= (1LL << 40) || d->C > (1 << 24)) return GPP_ERR_UNSUPPORTED;
    if ((uintptr_t)d->in & 3 || (uintptr_t)d->out & 3) return GPP_ERR_ALIGN;
    const float* base = (const float*)d->in + d->c_off;
    if (d->layout != GPP_ABSMAX_F32) {
        // a split row is a sequence of 128-byte channel groups: whole groups only, on 128-byte boundaries
        if (d->C % 32 != 0 || d->pitch % 32 != 0 || d->c_off % 32 != 0) return GPP_ERR_BAD_ARG;
        if ((uintptr_t)d->in & 127) return GPP_ERR_ALIGN;
        if (d->M == 0) return GPP_OK;
        return d->layout == GPP_ABSMAX_SPLIT_F16 ? launch<8, true, false>(base, d->M, d->pitch, d->C / 8, d->out, stream)
                                                 : launch<8, true, true>(base, d->M, d->pitch, d->C / 8, d->out, stream);
    }
    if (d->M == 0) return GPP_OK;
    if (d->C % 4 == 0 && d->pitch % 4 == 0 && ((uintptr_t)base & 15) == 0) return launch<4, true, false>(base, d->M, d->pitch, d->C / 4, d->out, stream);
    return launch<1, false, false>(base, d->M, d->pitch, d->C, d->out, stream);
}

// uint32 table[n] = 0 on the stream (a plan op: a captured graph replays the clearing)
extern "C" int gpp_absmax_clear(uint32_t* table, int64_t n, void* stream)
{
    if (!table || n < 0) return GPP_ERR_BAD_ARG;
    if (n == 0) return GPP_OK;
    return (int)hipMemsetAsync(table, 0, (size_t)n * sizeof(uint32_t), (hipStream_t)stream);
}
