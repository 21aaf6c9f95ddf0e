// CLEAR-MOT scoring of tracks on gfx950 (MI355X): per frame the optimal one-to-one assignment of the tracker's rows to the labels -- the
// Hungarian method in its shortest-augmenting-path form on exact integer costs --, then per sequence the identity switches, fragmentations
// and the mostly-tracked / mostly-lost shares.  DESIGN.md section 4.29 is the specification, utils/mot_eval.py the host form,
// tests/mot_oracle.py the loop-written oracle; include/gpp.h has the contract.  The overlaps are gpp_kitti_overlaps_f64's, unchanged.
//
//   assign_kernel  one frame per workgroup of ONE wavefront.  The frame's square cost matrix (side n = max(G, T): G labels in play, T
//                  rows) lies in LDS as int32, n x n, sized by the launch's largest possible side -- 64 KiB at 128, 4 KiB up to 32, so that
//                  frames of typical size share a CU by the dozen.  Everything else of the assignment lives in registers: lane l owns the
//                  columns l and l + 64 (their potential v, the row they hold, minv, way, used) and the rows l and l + 64 (their potential u
//                  and whether the row is in the current tree).  One step of the n^2 dependent steps is: read the line of the matrix, relax
//                  minv, reduce the packed key (minv << 8 | column) over the 64 lanes with six DPP moves -- the smallest key is the smallest
//                  reduced cost, the first column of equals --, update the potentials.  No barrier inside the loop: the matrix is read-only
//                  there, and the step's results are uniform over the wavefront.  A workgroup form (two wavefronts, one column per thread)
//                  would pay a barrier and an LDS round trip per step to halve two columns' arithmetic; it was not built.
//                  The lists "label g of the frame" and "row t of the frame" are never stored: the labels in play and the live rows are two
//                  128-bit masks, a rank is a population count below a bit.
//                  After the assignment the matrix is dead and its first 2.5 KiB hold five 128-entry tables that carry the result from
//                  the column owners to the label owners and the row owners.
//   clear_kernel   one workgroup of 128 threads per sequence, thread a is label slot a.  The frames are walked in order; a trajectory's
//                  state (last matched id, flags, counting frames, matched frames, switches, fragmentations) lies in LDS, up to
//                  GPP_MOT_MAX_TRAJECTORIES per sequence (21 KiB).  A label counts at most once per frame and trajectory, so no two
//                  threads touch one trajectory between two barriers.  The sequence's sums are integer atomics in LDS.
//
// Every loop bound is a function of the sizes; there is no spin wait and no word passes between workgroups.  Integers throughout: int64
// potentials (below 2^35), int32 costs; the only floating-point operations are the float64 compare against min_overlap and
// floor(overlap * 2^20).  No floating-point atomics.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"
#include "mot_assign.h"

namespace {

using namespace gpp_mot;                                // kWave, rank_below, read_lane, read_lane64, wave_min, wave_sum

constexpr int kMax = GPP_KITTI_MAX_DETECTIONS;          // rows and labels per frame
constexpr int kRow = GPP_POSE_COLS;
constexpr int kLabel = GPP_KITTI_LABEL_COLS;
constexpr int kScale = 1 << GPP_MOT_SCALE_BITS;
constexpr int kBig = GPP_MOT_BIG;
constexpr int kTraj = GPP_MOT_MAX_TRAJECTORIES;
constexpr int kClearThreads = 128;
constexpr int kTables = 5 * kMax;                       // int32 words the outcome phase needs of the dead matrix
constexpr size_t kSeqBytes = 256;

static_assert(kMax == GPP_KITTI_MAX_LABELS && kMax == 2 * kWave, "two columns and two rows per lane");
static_assert((long long)kMax * kScale < (long long)kBig, "most admissible pairs first, then the largest sum of k");
static_assert(kClearThreads == kMax, "one thread per label slot");

enum { L_NONE = 0, L_TP, L_FN, L_IGNORED_MATCHED, L_IGNORED_UNMATCHED };
enum { R_NONE = 0, R_TP, R_IGNORED, R_FP, R_LOW, R_DONTCARE };
enum { S_COUNTING = 0, S_IGNORED, S_DONTCARE, S_OUT };

__global__ __launch_bounds__(kWave) void assign_kernel(const double* __restrict__ overlaps, const double* __restrict__ labels,
                                                       const int32_t* __restrict__ label_counts, const float* __restrict__ rows,
                                                       const int32_t* __restrict__ ids, int D, int A, gpp_mot_params prm,
                                                       int32_t* __restrict__ match, int32_t* __restrict__ label_outcome,
                                                       int32_t* __restrict__ row_outcome, int64_t* __restrict__ frame_counts)
{
    extern __shared__ int32_t s_cost[];                  // n x n; afterwards five tables of kMax words

    const int f = blockIdx.x, lane = threadIdx.x;
    int count = A > 0 ? label_counts[f] : 0;
    count = count < 0 ? 0 : (count > A ? A : count);

    // ---- the labels' status and the live rows, two of each per lane; the masks
    int l_stat[2];
    bool r_live[2];
    double r_height[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int a = lane + kWave * s;
        l_stat[s] = S_OUT;
        if (a < count) {
            const double* g = labels + ((size_t)f * A + a) * kLabel;
            const double kind = g[0], trunc = g[1], occ = g[2], height = fabs(g[7] - g[5]);
            if (kind == 0.0) l_stat[s] = (occ > prm.max_occlusion || trunc > prm.max_truncation || height < prm.min_height) ? S_IGNORED : S_COUNTING;
            else if (kind == 1.0) l_stat[s] = S_IGNORED;
            else if (kind == 2.0) l_stat[s] = S_DONTCARE;
        }
        const int d = lane + kWave * s;
        r_live[s] = false;
        r_height[s] = 0.0;
        if (d < D) {
            const float* r = rows + ((size_t)f * D + d) * kRow;
            r_live[s] = r[14] >= 0.0f && ids[(size_t)f * D + d] >= 0;
            r_height[s] = fabs((double)r[29] - (double)r[27]);
        }
    }
    const unsigned long long g_lo = __ballot(l_stat[0] <= S_IGNORED), g_hi = __ballot(l_stat[1] <= S_IGNORED);
    const unsigned long long c_lo = __ballot(l_stat[0] == S_COUNTING), c_hi = __ballot(l_stat[1] == S_COUNTING);
    const unsigned long long dc_lo = __ballot(l_stat[0] == S_DONTCARE), dc_hi = __ballot(l_stat[1] == S_DONTCARE);
    const unsigned long long t_lo = __ballot(r_live[0]), t_hi = __ballot(r_live[1]);
    const int G = __popcll(g_lo) + __popcll(g_hi), T = __popcll(t_lo) + __popcll(t_hi);
    const int n = G > T ? G : T;                         // (<= max(D, A): the matrix fits the launch's allocation)

    // ---- the cost matrix: BIG everywhere, then the admissible pairs
    for (int c = lane; c < n * n; c += kWave) s_cost[c] = kBig;
    __syncthreads();
    if (G > 0 && T > 0) {
        const double* plane = overlaps + ((size_t)f * 4 + prm.metric) * D * A;
        for (int c = lane; c < D * count; c += kWave) {
            const int d = c / count, a = c - d * count;
            const bool in_play = ((a < 64 ? g_lo >> a : g_hi >> (a - 64)) & 1ull) != 0ull;
            const bool live = ((d < 64 ? t_lo >> d : t_hi >> (d - 64)) & 1ull) != 0ull;
            if (!in_play || !live) continue;
            const double o = plane[(size_t)d * A + a];
            if (!(o >= prm.min_overlap)) continue;       // (false for NaN)
            double x = o * (double)kScale;
            x = x > (double)kScale ? (double)kScale : x; // (an overlap above 1 -- boxes of negative sides -- counts as 1)
            const int k = (int)floor(x);
            s_cost[rank_below(g_lo, g_hi, a) * n + rank_below(t_lo, t_hi, d)] = kScale - k;
        }
    }
    __syncthreads();

    // ---- the assignment: rows in order, each by a shortest augmenting path.  Column j = lane + 64 s, row r = lane + 64 s
    long long u[2] = {0, 0}, v[2] = {0, 0};
    int p[2] = {-1, -1};                                 // the row a column holds
    for (int i = 0; i < n; ++i) {
        long long minv[2];
        int way[2] = {-1, -1};
        bool used[2] = {false, false}, in_tree[2] = {false, false};
        minv[0] = minv[1] = INT64_MAX;
        int i0 = i, j0 = -1;                             // (j0 == -1: the virtual column that holds row i)
        for (int step = 0; step <= n; ++step) {          // (at most n columns join the tree)
            if (lane == (i0 & 63)) { if (i0 >> 6) in_tree[1] = true; else in_tree[0] = true; }
            const long long u0 = read_lane64(i0 >> 6 ? u[1] : u[0], i0 & 63);
            unsigned long long key = ~0ull;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = lane + kWave * s;
                if (j < n && !used[s]) {
                    const long long cur = (long long)s_cost[i0 * n + j] - u0 - v[s];
                    if (cur < minv[s]) { minv[s] = cur; way[s] = j0; }
                    const unsigned long long k = ((unsigned long long)minv[s] << 8) | (unsigned long long)j;      // (0 <= minv < 2^36)
                    key = k < key ? k : key;
                }
            }
            key = wave_min(key);
            const long long delta = (long long)(key >> 8);
            const int j1 = __builtin_amdgcn_readfirstlane((int)(key & 127ull));
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (used[s]) v[s] -= delta;
                else if (lane + kWave * s < n) minv[s] -= delta;
                if (in_tree[s]) u[s] += delta;
            }
            j0 = j1;
            if (lane == (j0 & 63)) { if (j0 >> 6) used[1] = true; else used[0] = true; }
            i0 = read_lane(j0 >> 6 ? p[1] : p[0], j0 & 63);
            if (i0 < 0) break;                           // a free column: the path ends here
        }
        for (int step = 0; step <= n && j0 >= 0; ++step) {                     // the path back: every column takes the row of the one before it
            const int j1 = read_lane(j0 >> 6 ? way[1] : way[0], j0 & 63);
            const int row = j1 < 0 ? i : read_lane(j1 >> 6 ? p[1] : p[0], j1 & 63);
            if (lane == (j0 & 63)) { if (j0 >> 6) p[1] = row; else p[0] = row; }
            j0 = j1;
        }
    }

    // ---- the matched cells, read before the matrix dies
    int cell[2] = {kBig, kBig};
    long long total = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = lane + kWave * s;
        if (j < n && p[s] >= 0) {
            cell[s] = s_cost[p[s] * n + j];
            total += cell[s];
        }
    }
    total = wave_sum(total);
    __syncthreads();
    int32_t* col_of_row = s_cost;                        // label g -> its column t, -1: none
    int32_t* cost_of_row = s_cost + kMax;
    int32_t* row_of_col = s_cost + 2 * kMax;             // column t -> its label g, -1: none
    int32_t* d_of_col = s_cost + 3 * kMax;               // column t -> the row index d
    int32_t* a_of_row = s_cost + 4 * kMax;               // label g -> the label index a
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        col_of_row[lane + kWave * s] = -1;
        row_of_col[lane + kWave * s] = -1;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int j = lane + kWave * s;
        if (j < T && p[s] >= 0 && p[s] < G && cell[s] < kBig) {                // (a pair at BIG is no pair)
            col_of_row[p[s]] = j;
            cost_of_row[p[s]] = cell[s];
            row_of_col[j] = p[s];
        }
        if (l_stat[s] <= S_IGNORED) a_of_row[rank_below(g_lo, g_hi, j)] = j;
        if (r_live[s]) d_of_col[rank_below(t_lo, t_hi, j)] = j;
    }
    __syncthreads();

    // ---- the outcomes
    long long sum_k = 0;
    bool is_tp[2], is_fn[2], is_fp[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int a = lane + kWave * s;
        is_tp[s] = is_fn[s] = is_fp[s] = false;
        if (a < A) {
            int m = -1, code = L_NONE;
            if (l_stat[s] <= S_IGNORED) {
                const int g = rank_below(g_lo, g_hi, a), t = col_of_row[g];
                if (t >= 0) {
                    m = d_of_col[t];
                    code = l_stat[s] == S_COUNTING ? L_TP : L_IGNORED_MATCHED;
                    if (l_stat[s] == S_COUNTING) { is_tp[s] = true; sum_k += kScale - cost_of_row[g]; }
                } else {
                    code = l_stat[s] == S_COUNTING ? L_FN : L_IGNORED_UNMATCHED;
                    is_fn[s] = l_stat[s] == S_COUNTING;
                }
            }
            match[(size_t)f * A + a] = m;
            label_outcome[(size_t)f * A + a] = code;
        }
        const int d = lane + kWave * s;
        if (d < D) {
            int code = R_NONE;
            if (r_live[s]) {
                const int g = row_of_col[rank_below(t_lo, t_hi, d)];
                if (g >= 0) {
                    const int a2 = a_of_row[g];
                    code = ((a2 < 64 ? c_lo >> a2 : c_hi >> (a2 - 64)) & 1ull) ? R_TP : R_IGNORED;
                } else if (r_height[s] < prm.min_height) {
                    code = R_LOW;
                } else {
                    code = R_FP;
                    const double* inside = overlaps + ((size_t)f * 4 + 3) * D * A + (size_t)d * A;
                    for (int a2 = 0; a2 < count; ++a2)
                        if (((a2 < 64 ? dc_lo >> a2 : dc_hi >> (a2 - 64)) & 1ull) && inside[a2] > 0.5) { code = R_DONTCARE; break; }
                    is_fp[s] = code == R_FP;
                }
            }
            row_outcome[(size_t)f * D + d] = code;
        }
    }
    sum_k = wave_sum(sum_k);
    const int tp = __popcll(__ballot(is_tp[0])) + __popcll(__ballot(is_tp[1]));
    const int fn = __popcll(__ballot(is_fn[0])) + __popcll(__ballot(is_fn[1]));
    const int fp = __popcll(__ballot(is_fp[0])) + __popcll(__ballot(is_fp[1]));
    if (lane == 0) {
        int64_t* out = frame_counts + (size_t)f * GPP_MOT_FRAME_COUNTS;
        out[0] = tp; out[1] = fp; out[2] = fn; out[3] = __popcll(c_lo) + __popcll(c_hi);
        out[4] = sum_k; out[5] = total; out[6] = G; out[7] = T;
    }
}

__global__ __launch_bounds__(kClearThreads) void clear_kernel(const int32_t* __restrict__ match, const int32_t* __restrict__ label_outcome,
                                                              const int32_t* __restrict__ traj, const int32_t* __restrict__ ids,
                                                              const int64_t* __restrict__ frame_counts, int N, int D, int A,
                                                              const int32_t* __restrict__ seq_start, int max_traj,
                                                              int64_t* __restrict__ seq_counts, int32_t* __restrict__ traj_table)
{
    __shared__ int32_t t_last[kTraj], t_counting[kTraj], t_matched[kTraj], t_ids[kTraj], t_frag[kTraj];
    __shared__ unsigned char t_flags[kTraj];             // 1: matched before, 2: its last counting frame was unmatched
    __shared__ unsigned long long s_sum[GPP_MOT_SEQ_COUNTS];

    const int seq = blockIdx.x, tid = threadIdx.x;
    int f0 = seq_start[seq], f1 = seq_start[seq + 1];
    f0 = f0 < 0 ? 0 : f0;                                // (the host has checked the ranges; no frame index leaves [0, N) whatever arrives)
    f1 = f1 > N ? N : f1;
    for (int t = tid; t < max_traj; t += kClearThreads) {
        t_last[t] = -1; t_counting[t] = 0; t_matched[t] = 0; t_ids[t] = 0; t_frag[t] = 0; t_flags[t] = 0;
    }
    if (tid < GPP_MOT_SEQ_COUNTS) s_sum[tid] = 0ull;
    __syncthreads();

    // ---- the frames' sums
    {
        long long part[6] = {0, 0, 0, 0, 0, 0};
        for (int f = f0 + tid; f < f1; f += kClearThreads)
#pragma unroll
            for (int k = 0; k < 6; ++k) part[k] += frame_counts[(size_t)f * GPP_MOT_FRAME_COUNTS + k];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (part[k] != 0) atomicAdd(&s_sum[k], (unsigned long long)part[k]);
    }

    // ---- the trajectories, frame by frame
    for (int f = f0; f < f1; ++f) {
        if (tid < A) {
            const int code = label_outcome[(size_t)f * A + tid];
            const int t = traj[(size_t)f * A + tid];
            if ((code == L_TP || code == L_FN) && t >= 0 && t < max_traj) {
                t_counting[t] += 1;
                unsigned flags = t_flags[t];
                if (code == L_TP) {
                    const int d = match[(size_t)f * A + tid];
                    const int id = d >= 0 && d < D ? ids[(size_t)f * D + d] : -1;
                    t_matched[t] += 1;
                    if (flags & 1u) {
                        if (t_last[t] != id) t_ids[t] += 1;
                        if (flags & 2u) t_frag[t] += 1;
                    }
                    t_last[t] = id;
                    flags = 1u;
                } else {
                    flags |= 2u;
                }
                t_flags[t] = (unsigned char)flags;
            }
        }
        __syncthreads();
    }

    // ---- the table and the sequence's counts
    {
        unsigned long long n_ids = 0, n_frag = 0, mt = 0, pt = 0, ml = 0, n_traj = 0;
        for (int t = tid; t < max_traj; t += kClearThreads) {
            const int counting = t_counting[t], matched = t_matched[t];
            int32_t* line = traj_table + ((size_t)seq * max_traj + t) * GPP_MOT_TRAJ_COLS;
            line[0] = counting; line[1] = matched; line[2] = t_ids[t]; line[3] = t_frag[t];
            if (counting == 0) continue;
            n_traj += 1; n_ids += t_ids[t]; n_frag += t_frag[t];
            if (5 * matched >= 4 * counting) mt += 1;    // matched / counting >= 0.8, in integers
            else if (5 * matched < counting) ml += 1;    // < 0.2
            else pt += 1;
        }
        if (n_ids) atomicAdd(&s_sum[6], n_ids);
        if (n_frag) atomicAdd(&s_sum[7], n_frag);
        if (mt) atomicAdd(&s_sum[8], mt);
        if (pt) atomicAdd(&s_sum[9], pt);
        if (ml) atomicAdd(&s_sum[10], ml);
        if (n_traj) atomicAdd(&s_sum[11], n_traj);
    }
    __syncthreads();
    if (tid < GPP_MOT_SEQ_COUNTS) seq_counts[(size_t)seq * GPP_MOT_SEQ_COUNTS + tid] = tid == 12 ? (int64_t)(f1 > f0 ? f1 - f0 : 0) : (int64_t)s_sum[tid];
}

size_t seq_bytes(int S) { return ((size_t)(S + 1) * sizeof(int32_t) + kSeqBytes - 1) / kSeqBytes * kSeqBytes; }

}  // namespace

extern "C" int gpp_mot_assign(const double* overlaps, const double* labels, const int32_t* label_counts, const float* rows,
                              const int32_t* ids, int N, int D, int A, const gpp_mot_params* params, int32_t* match,
                              int32_t* label_outcome, int32_t* row_outcome, int64_t* frame_counts, void* stream)
{
    if (N < 0 || D < 0 || A < 0 || !params) return GPP_ERR_BAD_ARG;
    const gpp_mot_params& p = *params;
    if (p.metric < 0 || p.metric > 2 || p.reserved != 0) return GPP_ERR_BAD_ARG;
    if (!(p.min_overlap >= 0.0 && p.min_overlap <= 1.0)) return GPP_ERR_BAD_ARG;
    if (__builtin_isnan(p.max_occlusion) || __builtin_isnan(p.max_truncation) || __builtin_isnan(p.min_height)) return GPP_ERR_BAD_ARG;
    if (D > kMax || A > kMax) return GPP_ERR_UNSUPPORTED;
    if (N == 0) return GPP_OK;
    if (!frame_counts) return GPP_ERR_BAD_ARG;
    if (A > 0 && (!labels || !label_counts || !match || !label_outcome)) return GPP_ERR_BAD_ARG;
    if (D > 0 && (!rows || !ids || !row_outcome)) return GPP_ERR_BAD_ARG;
    if (D > 0 && A > 0 && !overlaps) return GPP_ERR_BAD_ARG;
    const int side = D > A ? D : A;
    const int words = side * side > kTables ? side * side : kTables;
    assign_kernel<<<dim3((unsigned)N), dim3(kWave), (size_t)words * sizeof(int32_t), (hipStream_t)stream>>>(
        overlaps, labels, label_counts, rows, ids, D, A, p, match, label_outcome, row_outcome, frame_counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_mot_clear_workspace_bytes(int S, size_t* bytes)
{
    if (S < 0 || !bytes) return GPP_ERR_BAD_ARG;
    *bytes = seq_bytes(S);
    return GPP_OK;
}

extern "C" int gpp_mot_clear(const int32_t* match, const int32_t* label_outcome, const int32_t* traj, const int32_t* ids,
                             const int64_t* frame_counts, int N, int D, int A, const int32_t* seq_start, int S, int max_traj,
                             int64_t* seq_counts, int32_t* traj_table, void* workspace, size_t workspace_bytes, void* stream)
{
    if (N < 0 || D < 0 || A < 0 || S < 0 || max_traj < 0 || !seq_start) return GPP_ERR_BAD_ARG;
    for (int s = 0; s <= S; ++s) {
        const int32_t lo = s == 0 ? 0 : seq_start[s - 1];
        if (seq_start[s] < lo || seq_start[s] > N) return GPP_ERR_BAD_ARG;
    }
    if (D > kMax || A > kMax || max_traj > kTraj) return GPP_ERR_UNSUPPORTED;
    if (S == 0) return GPP_OK;
    if (!seq_counts || !workspace || (max_traj > 0 && !traj_table)) return GPP_ERR_BAD_ARG;
    if (N > 0 && !frame_counts) return GPP_ERR_BAD_ARG;
    if (N > 0 && A > 0 && (!match || !label_outcome || !traj)) return GPP_ERR_BAD_ARG;
    if (N > 0 && D > 0 && !ids) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)workspace & 3u) return GPP_ERR_ALIGN;
    if (workspace_bytes < seq_bytes(S)) return GPP_ERR_WORKSPACE;
    hipStream_t q = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(workspace, seq_start, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, q);
    if (e != hipSuccess) return (int)e;
    clear_kernel<<<dim3((unsigned)S), dim3(kClearThreads), 0, q>>>(match, label_outcome, traj, ids, frame_counts, N, D, A,
                                                                   (const int32_t*)workspace, max_traj, seq_counts, traj_table);
    e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
