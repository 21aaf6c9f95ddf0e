// HOTA scoring of tracks on gfx950 (MI355X): the alignment score of every (label trajectory, tracker id) pair of a sequence, per frame the
// optimal one-to-one assignment of the kept rows to the counting labels on costs that this score weighs, and per sequence the detection,
// association and localisation integers at the 19 thresholds 0.05 .. 0.95.  DESIGN.md section 4.30 is the specification, utils/hota_eval.py
// the host form, tests/hota_oracle.py the loop-written oracle; include/gpp.h has the contract.  The overlaps are gpp_kitti_overlaps_f64's and
// the codes gpp_mot_assign's, both unchanged: a label COUNTS iff its label_outcome is 1 or 2, a row is KEPT iff its row_outcome is 1 or 3.
//
//   potential_kernel  pass 1, one frame per workgroup of 256 threads.  The frame's similarities q = floor(min(o 2^20, 2^20)) lie in LDS
//                     (21 bits each, kept as a 16-bit and an 8-bit plane: 48 KiB at 128 x 128, so that the launch stays inside the 64 KiB a
//                     kernel gets without asking), with the row sums rs, the column sums cs and the frame's (trajectory, tracker) indices.
//                     Every pair with q > 0 adds floor(q 2^20 / (rs + cs - q)) to its cell of the sequence's pair table P by a 64-bit
//                     integer atomic; every counting label and kept row adds 1 to gc / tc by a 32-bit one.
//   match_kernel      pass 2, one frame per workgroup of ONE wavefront, the shape of mot_eval.hip's assign_kernel: the int32 matrix in LDS,
//                     sized by the launch's largest side, two columns per lane, the arg-min by the DPP reduction of the packed key --
//                     csrc/mot_assign.h is that routine.  A cell is 2^20 - ((A q) >> 20) with A = floor(P 2^20 / ((gc + tc) 2^20 - P)) formed
//                     on the fly from the finished table (and written out: every frame that touches a cell writes the same value).
//                     After the assignment the matrix is dead and its first 1.5 KiB carry the result from the column owners to the label
//                     owners.  A pair of the assignment with jm = min(19, (20 q + 19) >> 20) >= 1 counts: hist[cell][jm] += 1 (32-bit
//                     atomic), TP_j and SQ_j for j <= jm.
//   reduce_kernel     one thread per cell of a sequence's table, grid (blocks, sequences): the suffix sums of the cell's counters, three
//                     int64 quotients per threshold, a wavefront sum and one 64-bit integer atomic per wavefront and quantity; the
//                     wavefronts also sum the sequence's frame_hota columns.
//
// Pass 2 reads what EVERY frame of the sequence added in pass 1: the caller runs gpp_hota_potential on all chunks before gpp_hota_match on
// any, on one stream.  Every loop bound is a function of the sizes; there is no spin wait and no word passes between workgroups of one
// launch.  Integers throughout; the only floating-point operation is floor(overlap * 2^20).  No floating-point atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"
#include "mot_assign.h"
#include "pair_tables.h"

namespace {

using namespace gpp_mot;                                // kWave, rank_below, wave_sum, assign_rows
using namespace gpp_pairs;                              // kScaleBits, kScale, kTabCols, kSeqTabCols, quantise and the host checks

constexpr int kMax = GPP_KITTI_MAX_DETECTIONS;          // rows and labels per frame
constexpr int kLevels = GPP_HOTA_LEVELS;                // the thresholds j / 20, j = 1 .. 19
constexpr int kHist = GPP_HOTA_HIST;                    // counters per cell: index jm, 0 unused
constexpr int kFrameCols = GPP_HOTA_FRAME_COLS;
constexpr int kSeqCols = GPP_HOTA_SEQ_COLS;
constexpr int kPotThreads = 256;
constexpr int kRedThreads = 256;
constexpr int kTables = 3 * kMax;                       // int32 words the outcome phase needs of the dead matrix

static_assert(kMax == GPP_KITTI_MAX_LABELS && kMax == 2 * kWave, "two columns and two rows per lane");
static_assert(kPotThreads == 2 * kMax, "one thread per label and one per row");
static_assert(kHist == kLevels + 1 && kHist % 4 == 0, "a cell's counters are five 16-byte words");
static_assert(kFrameCols == 2 * kLevels + 2, "TP and SQ per threshold, G' and T'");
static_assert(3 * kMax * kMax + 4 * kMax * 4 <= 65536, "pass 1 stays inside 64 KiB of LDS");

__device__ __forceinline__ bool bit_of(unsigned long long lo, unsigned long long hi, int i)
{
    return ((i < 64 ? lo >> i : hi >> (i - 64)) & 1ull) != 0ull;
}

__global__ __launch_bounds__(kPotThreads) void potential_kernel(const double* __restrict__ overlaps, const int32_t* __restrict__ label_outcome,
                                                                const int32_t* __restrict__ row_outcome, const int32_t* __restrict__ traj,
                                                                const int32_t* __restrict__ trk, int D, int A, int metric,
                                                                const int32_t* __restrict__ tab, unsigned long long* __restrict__ P,
                                                                int32_t* __restrict__ cnt)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    int32_t* s_rs = (int32_t*)s_raw;                     // [kMax] the sum of q over the rows, per label
    int32_t* s_cs = s_rs + kMax;                         // [kMax] the sum of q over the labels, per row
    int32_t* s_g = s_cs + kMax;                          // [kMax] a counting label's trajectory, -1 otherwise
    int32_t* s_t = s_g + kMax;                           // [kMax] a kept row's tracker index, -1 otherwise
    uint16_t* s_lo = (uint16_t*)(s_t + kMax);            // [D * A] q's low 16 bits
    unsigned char* s_hi = (unsigned char*)(s_lo + D * A);                      // [D * A] q's bits 16 .. 20

    const int f = blockIdx.x, tid = threadIdx.x;
    const int cell_base = tab[(size_t)f * kTabCols], n_gt = tab[(size_t)f * kTabCols + 1], n_trk = tab[(size_t)f * kTabCols + 2];
    const int vec_base = tab[(size_t)f * kTabCols + 3];

    if (tid < kMax) {
        int g = -1;
        if (tid < A) {
            const int code = label_outcome[(size_t)f * A + tid], t = traj[(size_t)f * A + tid];
            if ((code == 1 || code == 2) && t >= 0 && t < n_gt) g = t;
        }
        s_g[tid] = g;
    } else {
        const int d = tid - kMax;
        int t = -1;
        if (d < D) {
            const int code = row_outcome[(size_t)f * D + d], k = trk[(size_t)f * D + d];
            if ((code == 1 || code == 3) && k >= 0 && k < n_trk) t = k;
        }
        s_t[d] = t;
    }
    __syncthreads();

    const int cells = D * A;
    const double* plane = overlaps + ((size_t)f * 4 + metric) * (size_t)cells;
    for (int c = tid; c < cells; c += kPotThreads) {
        const int d = c / A, a = c - d * A;
        const int q = (s_g[a] >= 0 && s_t[d] >= 0) ? quantise(plane[c]) : 0;
        s_lo[c] = (uint16_t)(q & 0xffff);
        s_hi[c] = (unsigned char)(q >> 16);
    }
    __syncthreads();

    if (tid < kMax) {
        const int a = tid;
        int sum = 0;
        if (a < A)
            for (int d = 0; d < D; ++d) sum += (int)s_lo[d * A + a] | ((int)s_hi[d * A + a] << 16);
        s_rs[a] = sum;                                   // (<= 128 * 2^20)
        if (a < A && s_g[a] >= 0) atomicAdd(&cnt[(size_t)vec_base + s_g[a]], 1);
    } else {
        const int d = tid - kMax;
        int sum = 0;
        if (d < D)
            for (int k = 0; k < A; ++k) {                // (label (k + d) mod A first: the threads of a wavefront read different banks)
                const int a = (k + d) % A;
                sum += (int)s_lo[d * A + a] | ((int)s_hi[d * A + a] << 16);
            }
        s_cs[d] = sum;
        if (d < D && s_t[d] >= 0) atomicAdd(&cnt[(size_t)vec_base + n_gt + s_t[d]], 1);
    }
    __syncthreads();

    for (int c = tid; c < cells; c += kPotThreads) {
        const int q = (int)s_lo[c] | ((int)s_hi[c] << 16);
        if (q <= 0) continue;                            // (q > 0 only where the label counts and the row is kept)
        const int d = c / A, a = c - d * A;
        const unsigned long long den = (unsigned long long)(s_rs[a] + s_cs[d] - q);                 // (>= q > 0)
        const unsigned long long p = ((unsigned long long)q << kScaleBits) / den;                   // (numerator <= 2^40)
        atomicAdd(&P[(size_t)cell_base + (size_t)s_g[a] * n_trk + s_t[d]], p);
    }
}

__global__ __launch_bounds__(kWave) void match_kernel(const double* __restrict__ overlaps, const int32_t* __restrict__ label_outcome,
                                                      const int32_t* __restrict__ row_outcome, const int32_t* __restrict__ traj,
                                                      const int32_t* __restrict__ trk, int D, int A, int metric,
                                                      const int32_t* __restrict__ tab, const unsigned long long* __restrict__ P,
                                                      const int32_t* __restrict__ cnt, int32_t* __restrict__ align,
                                                      int32_t* __restrict__ hist, int32_t* __restrict__ match, int64_t* __restrict__ frame_hota)
{
    extern __shared__ __attribute__((aligned(16))) int32_t s_cost[];           // n x n; afterwards three tables of kMax words

    const int f = blockIdx.x, lane = threadIdx.x;
    const int cell_base = tab[(size_t)f * kTabCols], n_gt = tab[(size_t)f * kTabCols + 1], n_trk = tab[(size_t)f * kTabCols + 2];
    const int vec_base = tab[(size_t)f * kTabCols + 3];

    // ---- the counting labels and the kept rows, two of each per lane; the masks
    int g_of[2] = {-1, -1}, t_of[2] = {-1, -1};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = lane + kWave * s;
        if (i < A) {
            const int code = label_outcome[(size_t)f * A + i], t = traj[(size_t)f * A + i];
            if ((code == 1 || code == 2) && t >= 0 && t < n_gt) g_of[s] = t;
        }
        if (i < D) {
            const int code = row_outcome[(size_t)f * D + i], k = trk[(size_t)f * D + i];
            if ((code == 1 || code == 3) && k >= 0 && k < n_trk) t_of[s] = k;
        }
    }
    const unsigned long long c_lo = __ballot(g_of[0] >= 0), c_hi = __ballot(g_of[1] >= 0);
    const unsigned long long k_lo = __ballot(t_of[0] >= 0), k_hi = __ballot(t_of[1] >= 0);
    const int G = __popcll(c_lo) + __popcll(c_hi), T = __popcll(k_lo) + __popcll(k_hi);
    const int n = G > T ? G : T;                         // (<= max(D, A): the matrix fits the launch's allocation)

    // ---- the matrix: 2^20 everywhere, then the real pairs
    for (int c = lane; c < n * n; c += kWave) s_cost[c] = kScale;
    __syncthreads();
    const double* plane = overlaps + ((size_t)f * 4 + metric) * (size_t)D * A;
    if (G > 0 && T > 0) {
        for (int c = lane; c < D * A; c += kWave) {
            const int d = c / A, a = c - d * A;
            if (!bit_of(c_lo, c_hi, a) || !bit_of(k_lo, k_hi, d)) continue;
            const int q = quantise(plane[c]);
            const int g = traj[(size_t)f * A + a], t = trk[(size_t)f * D + d];
            const size_t cell = (size_t)cell_base + (size_t)g * n_trk + t;
            const long long pv = (long long)P[cell];
            long long av = 0;
            if (pv > 0) {
                const long long den = ((long long)(cnt[(size_t)vec_base + g] + cnt[(size_t)vec_base + n_gt + t]) << kScaleBits) - pv;
                av = den > 0 ? (long long)(((unsigned long long)pv << kScaleBits) / (unsigned long long)den) : 0;     // (P <= min(gc, tc) 2^20)
            }
            align[cell] = (int32_t)av;
            s_cost[rank_below(c_lo, c_hi, a) * n + rank_below(k_lo, k_hi, d)] = kScale - (int)((av * q) >> kScaleBits);
        }
    }
    __syncthreads();

    // ---- the assignment: section 4.29's routine
    int p[2];                                            // the row a column holds
    assign_rows(s_cost, n, lane, p);
    __syncthreads();

    int32_t* a_of_row = s_cost;                          // matrix row -> the label index a
    int32_t* d_of_col = s_cost + kMax;                   // matrix column -> the row index d
    int32_t* match_of = s_cost + 2 * kMax;               // label a -> the row it is paired with, -1: none
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = lane + kWave * s;
        match_of[i] = -1;
        if (g_of[s] >= 0) a_of_row[rank_below(c_lo, c_hi, i)] = i;
        if (t_of[s] >= 0) d_of_col[rank_below(k_lo, k_hi, i)] = i;
    }
    __syncthreads();

    // ---- the pairs, by the owners of their columns
    int jm[2] = {0, 0};
    long long qq[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = lane + kWave * s;
        if (j < T && p[s] >= 0 && p[s] < G) {
            const int a = a_of_row[p[s]], d = d_of_col[j];
            const int q = quantise(plane[(size_t)d * A + a]);
            int m = (20 * q + 19) >> kScaleBits;         // the largest j with floor(j 2^20 / 20) <= q
            m = m > kLevels ? kLevels : m;
            if (m >= 1) {
                jm[s] = m;
                qq[s] = q;
                match_of[a] = d;
                const int g = traj[(size_t)f * A + a], t = trk[(size_t)f * D + d];
                atomicAdd(&hist[((size_t)cell_base + (size_t)g * n_trk + t) * kHist + m], 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int a = lane + kWave * s;
        if (a < A) match[(size_t)f * A + a] = match_of[a];
    }
    int64_t* out = frame_hota + (size_t)f * kFrameCols;
    for (int j = 1; j <= kLevels; ++j) {
        const int tp = __popcll(__ballot(jm[0] >= j)) + __popcll(__ballot(jm[1] >= j));
        const long long sq = wave_sum((jm[0] >= j ? qq[0] : 0ll) + (jm[1] >= j ? qq[1] : 0ll));
        if (lane == 0) { out[j - 1] = tp; out[kLevels + j - 1] = sq; }
    }
    if (lane == 0) { out[2 * kLevels] = G; out[2 * kLevels + 1] = T; }
}

__global__ __launch_bounds__(kRedThreads) void reduce_kernel(const int64_t* __restrict__ frame_hota, int N, const int32_t* __restrict__ seq_tab,
                                                             const int32_t* __restrict__ hist, const int32_t* __restrict__ cnt,
                                                             unsigned long long* __restrict__ seq_hota)
{
    const int seq = blockIdx.y, lane = threadIdx.x & (kWave - 1);
    const int32_t* st = seq_tab + (size_t)seq * kSeqTabCols;
    const int cell_base = st[0], n_gt = st[1], n_trk = st[2], vec_base = st[3];
    int f0 = st[4], f1 = st[5];
    f0 = f0 < 0 ? 0 : f0;                                // (the host has checked the ranges; no frame index leaves [0, N) whatever arrives)
    f1 = f1 > N ? N : f1;
    unsigned long long* out = seq_hota + (size_t)seq * kLevels * kSeqCols;
    const long long cells = (long long)n_gt * n_trk;
    const long long stride = (long long)gridDim.x * kRedThreads;

    // ---- the pair table: a wavefront takes 64 neighbouring cells at a time
    for (long long first = (long long)blockIdx.x * kRedThreads + (threadIdx.x - lane); first < cells; first += stride) {
        const long long c = first + lane;
        const int32_t* h = hist + ((size_t)cell_base + (size_t)(c < cells ? c : 0)) * kHist;
        int any = 0;
        if (c < cells) {
            const int4* h4 = (const int4*)h;             // (20 counters: five 16-byte words; the table is 16-byte aligned)
#pragma unroll
            for (int k = 0; k < kHist / 4; ++k) { const int4 w = h4[k]; any |= w.x | w.y | w.z | w.w; }
        }
        if (__ballot(any != 0) == 0ull) continue;
        long long gc = 1, tc = 1;
        if (any) {
            const int g = (int)(c / n_trk), t = (int)(c - (long long)g * n_trk);
            gc = cnt[(size_t)vec_base + g];
            tc = cnt[(size_t)vec_base + n_gt + t];
        }
        long long mc = 0;
#pragma unroll 1
        for (int j = kLevels; j >= 1; --j) {
            if (any) mc += h[j];
            long long ass = 0, assre = 0, asspr = 0;
            if (mc > 0 && gc > 0 && tc > 0 && gc + tc > mc) {
                const unsigned long long num = (unsigned long long)(mc * mc) << kScaleBits;         // (mc <= 2^20 frames: below 2^60)
                ass = (long long)(num / (unsigned long long)(gc + tc - mc));
                assre = (long long)(num / (unsigned long long)gc);
                asspr = (long long)(num / (unsigned long long)tc);
            }
            if (__ballot(mc > 0) == 0ull) continue;
            ass = wave_sum(ass);
            assre = wave_sum(assre);
            asspr = wave_sum(asspr);
            if (lane == 0) {
                atomicAdd(&out[(j - 1) * kSeqCols + 4], (unsigned long long)ass);
                atomicAdd(&out[(j - 1) * kSeqCols + 5], (unsigned long long)assre);
                atomicAdd(&out[(j - 1) * kSeqCols + 6], (unsigned long long)asspr);
            }
        }
    }

    // ---- the frames' sums: a wavefront takes a column of frame_hota at a time
    const int n_waves = (int)gridDim.x * (kRedThreads / kWave);
    for (int k = (int)blockIdx.x * (kRedThreads / kWave) + (threadIdx.x >> 6); k < kFrameCols; k += n_waves) {
        long long sum = 0;
        for (int f = f0 + lane; f < f1; f += kWave) sum += frame_hota[(size_t)f * kFrameCols + k];
        sum = wave_sum(sum);
        if (sum == 0) continue;
        const unsigned long long plus = (unsigned long long)sum, minus = 0ull - plus;               // (two's complement: FN = sum G' - TP)
        if (k < kLevels) {
            if (lane == 0) {
                atomicAdd(&out[k * kSeqCols + 0], plus);
                atomicAdd(&out[k * kSeqCols + 1], minus);
                atomicAdd(&out[k * kSeqCols + 2], minus);
            }
        } else if (k < 2 * kLevels) {
            if (lane == 0) atomicAdd(&out[(k - kLevels) * kSeqCols + 3], plus);
        } else if (lane < kLevels) {
            atomicAdd(&out[lane * kSeqCols + (k == 2 * kLevels ? 1 : 2)], plus);
        }
    }
}

struct Layout { size_t align, hist, cnt, tab; };         // byte offsets into the workspace; P lies at 0

Layout layout_of(long long cells, long long vecs)
{
    Layout l;
    l.align = (size_t)cells * 8;
    l.hist = (size_t)cells * 12;                         // (a multiple of 16 iff cells is a multiple of 4: rounded below)
    l.hist = (l.hist + 15) / 16 * 16;
    l.cnt = l.hist + (size_t)cells * kHist * 4;
    l.tab = tab_offset(l.cnt, vecs);
    return l;
}

}  // namespace

extern "C" int gpp_hota_workspace_bytes(long long cells, long long vecs, int max_frames, int S, size_t* bytes)
{
    return workspace_size(cells, vecs, max_frames, S, layout_of(cells, vecs).tab, bytes);
}

extern "C" int gpp_hota_potential(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
                                  const int32_t* trk, int N, int D, int A, int metric, const int32_t* frame_tab, long long cells,
                                  long long vecs, void* workspace, size_t workspace_bytes, void* stream)
{
    const Layout l = layout_of(cells, vecs);
    bool launch;
    const int rc = check_frames(overlaps, label_outcome, row_outcome, traj, trk, N, D, A, metric, frame_tab, cells, vecs, l.tab, workspace,
                                workspace_bytes, &launch);
    if (rc != GPP_OK || !launch) return rc;
    unsigned char* w = (unsigned char*)workspace;
    hipStream_t q = (hipStream_t)stream;
    hipError_t e = upload_lines(w, l.tab, frame_tab, N, kTabCols, q);
    if (e != hipSuccess) return (int)e;
    const size_t lds = (size_t)4 * kMax * sizeof(int32_t) + (size_t)3 * D * A;
    potential_kernel<<<dim3((unsigned)N), dim3(kPotThreads), lds, q>>>(overlaps, label_outcome, row_outcome, traj, trk, D, A, metric,
                                                                      (const int32_t*)(w + l.tab), (unsigned long long*)w,
                                                                      (int32_t*)(w + l.cnt));
    return launched();
}

extern "C" int gpp_hota_match(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
                              const int32_t* trk, int N, int D, int A, int metric, const int32_t* frame_tab, long long cells,
                              long long vecs, int32_t* hota_match, int64_t* frame_hota, void* workspace, size_t workspace_bytes,
                              void* stream)
{
    const Layout l = layout_of(cells, vecs);
    bool launch;
    const int rc = check_frames(overlaps, label_outcome, row_outcome, traj, trk, N, D, A, metric, frame_tab, cells, vecs, l.tab, workspace,
                                workspace_bytes, &launch);
    if (rc != GPP_OK || !launch) return rc;
    if (!frame_hota || (A > 0 && !hota_match)) return GPP_ERR_BAD_ARG;
    unsigned char* w = (unsigned char*)workspace;
    hipStream_t q = (hipStream_t)stream;
    hipError_t e = upload_lines(w, l.tab, frame_tab, N, kTabCols, q);
    if (e != hipSuccess) return (int)e;
    const int side = D > A ? D : A;
    const int words = side * side > kTables ? side * side : kTables;
    match_kernel<<<dim3((unsigned)N), dim3(kWave), (size_t)words * sizeof(int32_t), q>>>(
        overlaps, label_outcome, row_outcome, traj, trk, D, A, metric, (const int32_t*)(w + l.tab), (const unsigned long long*)w,
        (const int32_t*)(w + l.cnt), (int32_t*)(w + l.align), (int32_t*)(w + l.hist), hota_match, frame_hota);
    return launched();
}

extern "C" int gpp_hota_reduce(const int64_t* frame_hota, int N, const int32_t* seq_tab, int S, long long cells, long long vecs,
                               int64_t* seq_hota, void* workspace, size_t workspace_bytes, void* stream)
{
    if (N < 0 || S < 0 || sizes_bad(cells, vecs)) return GPP_ERR_BAD_ARG;
    if (sizes_unsupported(cells, vecs) || S > 65535) return GPP_ERR_UNSUPPORTED;
    if (S == 0) return GPP_OK;
    if (!seq_tab || !seq_hota || !workspace || (N > 0 && !frame_hota)) return GPP_ERR_BAD_ARG;
    long long most = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* line = seq_tab + (size_t)s * kSeqTabCols;
        if (!line_ok(line, s ? line - kSeqTabCols : nullptr, cells, vecs)) return GPP_ERR_BAD_ARG;
        if (line[4] < (s ? line[5 - kSeqTabCols] : 0) || line[5] < line[4] || line[5] > N) return GPP_ERR_BAD_ARG;
        const long long n = (long long)line[1] * line[2];
        most = n > most ? n : most;
    }
    if ((uintptr_t)workspace & 15u) return GPP_ERR_ALIGN;
    const Layout l = layout_of(cells, vecs);
    if (workspace_bytes < l.tab + (size_t)S * kSeqTabCols * sizeof(int32_t)) return GPP_ERR_WORKSPACE;
    unsigned char* w = (unsigned char*)workspace;
    hipStream_t q = (hipStream_t)stream;
    hipError_t e = upload_lines(w, l.tab, seq_tab, S, kSeqTabCols, q);
    if (e != hipSuccess) return (int)e;
    long long blocks = (most + kRedThreads - 1) / kRedThreads;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    reduce_kernel<<<dim3((unsigned)blocks, (unsigned)S), dim3(kRedThreads), 0, q>>>(frame_hota, N, (const int32_t*)(w + l.tab),
                                                                                   (const int32_t*)(w + l.hist), (const int32_t*)(w + l.cnt),
                                                                                   (unsigned long long*)seq_hota);
    return launched();
}
