// Identity scoring of tracks (IDF1, IDR, IDP) on gfx950 (MI355X): per sequence the table C of how often every (label trajectory, tracker id)
// pair overlaps by at least one half, then ONE optimal assignment of the trajectories to the tracker ids on that table.  DESIGN.md section
// 4.31 is the specification, utils/idf1_eval.py the host form, tests/idf1_oracle.py the loop-written oracle; include/gpp.h has the contract.
// The overlaps are gpp_kitti_overlaps_f64's and the codes gpp_mot_assign's, both unchanged: a label COUNTS iff its label_outcome is 1 or 2,
// a row is KEPT iff its row_outcome is 1 or 3 -- HOTA's inputs (section 4.30).
//
//   count_kernel   pass 1, one frame per workgroup of 256 threads, the shape of hota_eval.hip's potential_kernel without the sums: every
//                  (counting label, kept row) pair with q = floor(min(o 2^20, 2^20)) >= 2^19 adds 1 to its cell of C, every counting label
//                  and kept row adds 1 to gc / tc, all by 32-bit integer atomics.
//   assign_kernel  pass 2, one sequence per workgroup of ONE wavefront.  The matrix is G x n, n = max(G, T) <= 4096: it stays where pass 1
//                  left it, in HBM -- the cell is 2^20 - C[g, t], formed on the fly; a padding column (t >= T) is 2^20 and reads nothing.
//                  Row i0 of a step is n_trk consecutive int32, and lane l owns the columns l, l + 64, ...: the read is coalesced.  The
//                  column state -- v, minv (int64), way, the row a column holds (int32): 24 bytes a column, 96 KiB at the cap -- and u
//                  (int64 per row, 8 KiB) lie in LDS, sized by the launch's largest sequence; which of its columns are used and which of
//                  its rows are in the tree a lane keeps as bit masks in registers (64 columns and 16 rows a lane at the most).  A lane
//                  reads and writes only its own words of v and minv.  u, way and the column's row are also read at an index that is the
//                  same in every lane (a broadcast): the wavefront's LDS operations run in the order they are issued, so there is no
//                  barrier anywhere in the dependent steps.  The arg-min is mot_assign.h's DPP reduction of the packed key
//                  minv << 13 | column.  The statements are section 4.29's, operation for operation: the potentials are updated in every
//                  step over the used and the unused columns as the rule states it.  A lane walks its columns eight at a time: the
//                  eight reads of a batch are issued without a branch around any of them (a column outside the matrix reads the last
//                  one's words and drops them), so that they are in flight together.  (Two more forms were built and measured, and
//                  taken out: one that first copied a table into LDS where it fits beside the state -- no gain at 100 x 300 --, and
//                  one that skipped the batch slots beyond a lane's last column by a uniform branch -- the loads of a batch were
//                  serialised again.  profiles/idf1/README.md has the figures.)
//
// Every loop bound is a function of the sizes; there is no spin wait and no word passes between workgroups of one launch.  Integers
// throughout; the only floating-point operation is floor(overlap * 2^20).  No floating-point atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include <atomic>

#include "gpp.h"
#include "mot_assign.h"
#include "pair_tables.h"

namespace {

using namespace gpp_mot;                                // kWave, read_lane, wave_min, wave_sum
using namespace gpp_pairs;                              // kScale, kTabCols, kSeqTabCols, quantise and the host checks

constexpr int kMax = GPP_KITTI_MAX_DETECTIONS;          // rows and labels per frame
constexpr int kHalf = kScale >> 1;
constexpr int kMaxRows = GPP_MOT_MAX_TRAJECTORIES;
constexpr int kMaxIds = GPP_IDF1_MAX_IDS;
constexpr int kSeqCols = GPP_IDF1_SEQ_COLS;
constexpr int kCountThreads = 256;
constexpr int kKeyBits = 13;                            // the column's bits of the packed key
constexpr int kBatch = 8;                              // columns of a lane whose reads are in flight together
constexpr int kColumnBytes = 24;                        // v, minv, way, the row it holds
constexpr size_t kLdsCap = (size_t)kMaxIds * kColumnBytes + (size_t)kMaxRows * 8;

static_assert(kMax == GPP_KITTI_MAX_LABELS && kCountThreads == 2 * kMax, "one thread per label and one per row");
static_assert(kMaxIds < (1 << kKeyBits) && kMaxIds % (kWave * kBatch) == 0 && kMaxIds / kWave <= 64, "a lane's columns fit a 64-bit mask, in whole batches");
static_assert(kMaxRows <= kMaxIds && kMaxRows % kWave == 0 && kMaxRows / kWave <= 32, "a lane's rows fit a 32-bit mask");
static_assert(kLdsCap <= 160 * 1024, "a gfx950 workgroup takes up to 160 KiB of LDS");

__global__ __launch_bounds__(kCountThreads) void count_kernel(const double* __restrict__ overlaps, const int32_t* __restrict__ label_outcome,
                                                              const int32_t* __restrict__ row_outcome, const int32_t* __restrict__ traj,
                                                              const int32_t* __restrict__ trk, int D, int A, int metric,
                                                              const int32_t* __restrict__ tab, int32_t* __restrict__ C,
                                                              int32_t* __restrict__ cnt)
{
    __shared__ int32_t s_g[kMax];                        // a counting label's trajectory, -1 otherwise
    __shared__ int32_t s_t[kMax];                        // a kept row's tracker index, -1 otherwise

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
        if (g >= 0) atomicAdd(&cnt[(size_t)vec_base + g], 1);
    } else {
        const int d = tid - kMax;
        int t = -1;
        if (d < D) {
            const int code = row_outcome[(size_t)f * D + d], k = trk[(size_t)f * D + d];
            if ((code == 1 || code == 3) && k >= 0 && k < n_trk) t = k;
        }
        s_t[d] = t;
        if (t >= 0) atomicAdd(&cnt[(size_t)vec_base + n_gt + t], 1);
    }
    __syncthreads();

    const int cells = D * A;
    const double* plane = overlaps + ((size_t)f * 4 + metric) * (size_t)cells;
    for (int c = tid; c < cells; c += kCountThreads) {
        const int d = c / A, a = c - d * A;
        const int g = s_g[a], t = s_t[d];
        if (g < 0 || t < 0) continue;
        if (quantise(plane[c]) >= kHalf) atomicAdd(&C[(size_t)cell_base + (size_t)g * n_trk + t], 1);
    }
}

__global__ __launch_bounds__(kWave) void assign_kernel(const int32_t* __restrict__ tab, const int32_t* __restrict__ C,
                                                       const int32_t* __restrict__ cnt, int n_cap, int32_t* __restrict__ id_match,
                                                       int64_t* __restrict__ seq_idf1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    long long* s_v = (long long*)s_raw;                                        // [n_cap] the column potentials
    long long* s_minv = s_v + n_cap;                                           // [n_cap]
    volatile long long* s_u = s_minv + n_cap;                                  // [g_cap] the row potentials (read by every lane)
    const int seq = blockIdx.x, lane = threadIdx.x;
    const int32_t* st = tab + (size_t)seq * kSeqTabCols;
    const int cell_base = st[0], G = st[1], T = st[2], vec_base = st[3];
    const int n = G > T ? G : T;
    const int g_cap = n_cap < kMaxRows ? n_cap : kMaxRows;
    volatile int32_t* s_p = (volatile int32_t*)(s_u + g_cap);                  // [n_cap] the row a column holds, -1: none
    volatile int32_t* s_way = s_p + n_cap;                                     // [n_cap] the column a column's minv came from
    int64_t* out = seq_idf1 + (size_t)seq * kSeqCols;

    // ---- the sums of the counters
    long long sum_gc = 0, sum_tc = 0;
    for (int g = lane; g < G; g += kWave) sum_gc += cnt[(size_t)vec_base + g];
    for (int t = lane; t < T; t += kWave) sum_tc += cnt[(size_t)vec_base + G + t];
    sum_gc = wave_sum(sum_gc);
    sum_tc = wave_sum(sum_tc);

    long long idtp = 0;
    if (G > 0 && T > 0 && n <= n_cap) {                  // (the host sized n_cap by the launch's largest sequence)
        const int K = (n + kWave - 1) / kWave;           // columns a lane owns, at the most
        for (int k = 0; k < K; ++k) {
            const int j = lane + kWave * k;
            if (j < n) { s_v[j] = 0; s_p[j] = -1; }
        }
        for (int g = lane; g < G; g += kWave) s_u[g] = 0;
        __builtin_amdgcn_wave_barrier();

        const int32_t* table = C + (size_t)cell_base;
        for (int i = 0; i < G; ++i) {
            unsigned long long used = 0ull;              // bit k: column lane + 64 k
            unsigned in_tree = 0u;                       // bit k: row lane + 64 k
            for (int k = 0; k < K; ++k) {
                const int j = lane + kWave * k;
                if (j < n) { s_minv[j] = INT64_MAX; s_way[j] = -1; }
            }
            int i0 = i, j0 = -1;                         // (j0 == -1: the virtual column that holds row i)
            for (int step = 0; step <= n; ++step) {      // (at most n columns join the tree)
                if (lane == (i0 & 63)) in_tree |= 1u << (i0 >> 6);
                const long long u0 = s_u[i0];
                const int32_t* line = table + (size_t)i0 * T;
                unsigned long long key = ~0ull;
                for (int k0 = 0; k0 < K; k0 += kBatch) {             // (a batch's reads are issued together, then used)
                    int count[kBatch];
                    long long v[kBatch], m[kBatch];
                    const unsigned taken = (unsigned)(used >> k0);             // (bit b: column lane + 64 (k0 + b))
#pragma unroll
                    for (int b = 0; b < kBatch; ++b) {
                        // (no lane-dependent branch around a read: a column outside the matrix reads the last one's words and drops them)
                        const int j = lane + kWave * (k0 + b), jt = j < T ? j : T - 1, jn = j < n ? j : n - 1;
                        count[b] = line[jt];
                        count[b] = j < T ? count[b] : 0;                        // (a padding column: 2^20 - 0)
                        v[b] = s_v[jn];
                        m[b] = s_minv[jn];
                    }
#pragma unroll
                    for (int b = 0; b < kBatch; ++b) {
                        const int j = lane + kWave * (k0 + b);
                        if (j < n && !((taken >> b) & 1u)) {
                            const long long cur = (long long)(kScale - count[b]) - u0 - v[b];
                            if (cur < m[b]) { m[b] = cur; s_minv[j] = cur; s_way[j] = j0; }
                            const unsigned long long kk = ((unsigned long long)m[b] << kKeyBits) | (unsigned long long)j;      // (0 <= minv < 2^33)
                            key = kk < key ? kk : key;
                        }
                    }
                }
                key = wave_min(key);
                if (key == ~0ull) { j0 = -1; break; }    // (no unused column: cannot happen, i < n columns hold a row)
                const long long delta = (long long)(key >> kKeyBits);
                const int j1 = __builtin_amdgcn_readfirstlane((int)(key & ((1ull << kKeyBits) - 1ull)));
                for (int k0 = 0; k0 < K; k0 += kBatch) {
                    long long* at[kBatch];               // a used column's v, an unused one's minv
                    long long w[kBatch];
                    const unsigned taken = (unsigned)(used >> k0);
#pragma unroll
                    for (int b = 0; b < kBatch; ++b) {
                        const int j = lane + kWave * (k0 + b), jn = j < n ? j : n - 1;
                        at[b] = (((taken >> b) & 1u) ? s_v : s_minv) + jn;
                        w[b] = *at[b];
                    }
#pragma unroll
                    for (int b = 0; b < kBatch; ++b)
                        if (lane + kWave * (k0 + b) < n) *at[b] = w[b] - delta;
                }
                for (unsigned rest = in_tree; rest; rest &= rest - 1u) {
                    const int g = lane + kWave * (__ffs(rest) - 1);
                    s_u[g] = s_u[g] + delta;
                }
                __builtin_amdgcn_wave_barrier();
                j0 = j1;
                if (lane == (j0 & 63)) used |= 1ull << (j0 >> 6);
                i0 = __builtin_amdgcn_readfirstlane(s_p[j0]);
                if (i0 < 0) break;                       // a free column: the path ends here
            }
            for (int step = 0; step <= n && j0 >= 0; ++step) {                 // the path back: every column takes the row of the one before it
                const int j1 = __builtin_amdgcn_readfirstlane(s_way[j0]);
                const int row = j1 < 0 ? i : __builtin_amdgcn_readfirstlane(s_p[j1]);
                if (lane == (j0 & 63)) s_p[j0] = row;
                __builtin_amdgcn_wave_barrier();
                j0 = j1;
            }
        }

        // ---- the pairs, by the owners of their columns
        for (int k = 0; k < K; ++k) {
            const int j = lane + kWave * k;
            if (j >= n) continue;
            const int g = s_p[j];
            if (g < 0) continue;
            const int c = j < T ? table[(size_t)g * T + j] : 0;
            id_match[(size_t)vec_base + g] = c > 0 ? j : -1;
            idtp += c > 0 ? c : 0;
        }
        idtp = wave_sum(idtp);
    } else {
        for (int g = lane; g < G; g += kWave) id_match[(size_t)vec_base + g] = -1;
    }
    if (lane == 0) {
        out[0] = idtp;
        out[1] = sum_gc - idtp;
        out[2] = sum_tc - idtp;
        out[3] = sum_gc;
        out[4] = sum_tc;
        out[5] = (long long)G * kScale - idtp;
        out[6] = G;
        out[7] = T;
    }
}

struct Layout { size_t cnt, tab; };                      // byte offsets into the workspace; C lies at 0

Layout layout_of(long long cells, long long vecs)
{
    Layout l;
    l.cnt = ((size_t)cells * 4 + 15) / 16 * 16;
    l.tab = tab_offset(l.cnt, vecs);
    return l;
}

}  // namespace

extern "C" int gpp_idf1_workspace_bytes(long long cells, long long vecs, int max_frames, int S, size_t* bytes)
{
    return workspace_size(cells, vecs, max_frames, S, layout_of(cells, vecs).tab, bytes);
}

extern "C" int gpp_idf1_count(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
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
    count_kernel<<<dim3((unsigned)N), dim3(kCountThreads), 0, q>>>(overlaps, label_outcome, row_outcome, traj, trk, D, A, metric,
                                                                   (const int32_t*)(w + l.tab), (int32_t*)w, (int32_t*)(w + l.cnt));
    return launched();
}

extern "C" int gpp_idf1_assign(const int32_t* seq_tab, int S, long long cells, long long vecs, int32_t* id_match, int64_t* seq_idf1,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    if (S < 0 || sizes_bad(cells, vecs)) return GPP_ERR_BAD_ARG;
    if (sizes_unsupported(cells, vecs)) return GPP_ERR_UNSUPPORTED;
    if (S == 0) return GPP_OK;
    if (!seq_tab || !seq_idf1 || !workspace) return GPP_ERR_BAD_ARG;
    int n_cap = 0;
    bool rows = false, beyond = false;
    for (int s = 0; s < S; ++s) {
        const int32_t* line = seq_tab + (size_t)s * kSeqTabCols;
        if (!line_ok(line, s ? line - kSeqTabCols : nullptr, cells, vecs)) return GPP_ERR_BAD_ARG;
        const int G = line[1], T = line[2], n = G > T ? G : T;
        beyond = beyond || G > kMaxRows || n > kMaxIds;
        rows = rows || G > 0;
        if (G > 0 && T > 0) n_cap = n > n_cap ? n : n_cap;
    }
    if (beyond) return GPP_ERR_UNSUPPORTED;
    if (rows && !id_match) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)workspace & 15u) return GPP_ERR_ALIGN;
    const Layout l = layout_of(cells, vecs);
    if (workspace_bytes < l.tab + (size_t)S * kSeqTabCols * sizeof(int32_t)) return GPP_ERR_WORKSPACE;
    n_cap = (n_cap + kWave - 1) / kWave * kWave;         // (keeps every LDS table 16-byte aligned)
    const size_t lds = (size_t)n_cap * kColumnBytes + (size_t)(n_cap < kMaxRows ? n_cap : kMaxRows) * 8;
    hipError_t e;
    if (lds > 64 * 1024) {
        // the dynamic-LDS attribute is per device: one bit per device ordinal (racing first calls set the same value)
        static std::atomic<uint64_t> configured{0};
        int dev = 0;
        e = hipGetDevice(&dev);
        if (e != hipSuccess) return (int)e;
        if (!(configured.load(std::memory_order_acquire) & (1ull << (dev & 63)))) {
            e = hipFuncSetAttribute((const void*)assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap);
            if (e != hipSuccess) return (int)e;
            configured.fetch_or(1ull << (dev & 63), std::memory_order_release);
        }
    }
    unsigned char* w = (unsigned char*)workspace;
    hipStream_t q = (hipStream_t)stream;
    e = upload_lines(w, l.tab, seq_tab, S, kSeqTabCols, q);
    if (e != hipSuccess) return (int)e;
    assign_kernel<<<dim3((unsigned)S), dim3(kWave), lds, q>>>((const int32_t*)(w + l.tab), (const int32_t*)w, (const int32_t*)(w + l.cnt),
                                                             n_cap, id_match, seq_idf1);
    return launched();
}
