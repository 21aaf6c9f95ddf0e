// What a pair table is, for the two scores that keep one per sequence -- csrc/hota_eval.hip (HOTA) and
// csrc/idf1_eval.hip (IDF1, section 4.31): a cell per (label trajectory, tracker id) pair and a counter per trajectory and per tracker id,
// found through table lines of host integers -- cell_base, n_gt, n_trk, vec_base per frame (kTabCols), those four and the frame range per
// sequence (kSeqTabCols).  A workspace holds the score's own tables first (each file's Layout) and ends in the copy of the lines that a
// call's kernel reads.  Here: the similarity q that fills a cell, and the host checks and the workspace tail that both files share.
// utils/pair_tables.py is the Python side of the same geometry.
//
// NOT here: which labels count and which rows are kept (the `code == 1 || code == 2 ...` staging of potential_kernel, match_kernel and
// count_kernel) and the kernels' read of a frame's line.  Both were tried as __forceinline__ helpers and changed the generated code
// (ten more SGPRs in match_kernel, reordered loads in count_kernel, another scalar schedule in potential_kernel's prologue), so the
// kernels keep their own text.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"

namespace gpp_pairs {

constexpr int kScaleBits = GPP_MOT_SCALE_BITS;
constexpr int kScale = 1 << kScaleBits;
constexpr int kTabCols = GPP_HOTA_TAB_COLS;
constexpr int kSeqTabCols = GPP_HOTA_SEQ_TAB_COLS;
constexpr long long kMaxCells = 1ll << 31;

// the similarity: floor(min(o 2^20, 2^20)), 0 for NaN and o <= 0 (section 4.29's k without the admissibility test)
__device__ __forceinline__ int quantise(double o)
{
    if (!(o > 0.0)) return 0;
    double x = o * (double)kScale;
    x = x > (double)kScale ? (double)kScale : x;
    return (int)floor(x);
}

inline bool sizes_bad(long long cells, long long vecs) { return cells < 0 || vecs < 0; }
inline bool sizes_unsupported(long long cells, long long vecs) { return cells >= kMaxCells || vecs >= kMaxCells; }

// a table line: cell_base, n_gt, n_trk, vec_base -- monotone bases, the cells and the counters inside the tables
inline bool line_ok(const int32_t* line, const int32_t* before, long long cells, long long vecs)
{
    const long long cell_base = line[0], n_gt = line[1], n_trk = line[2], vec_base = line[3];
    if (cell_base < 0 || n_gt < 0 || n_trk < 0 || vec_base < 0) return false;
    if (before && (cell_base < before[0] || vec_base < before[3])) return false;
    return cell_base + n_gt * n_trk <= cells && vec_base + n_gt + n_trk <= vecs;
}

// the byte offset of the lines' copy: behind `vecs` int32 counters that start at byte `cnt`, 16-byte aligned (the tail of a Layout)
inline size_t tab_offset(size_t cnt, long long vecs) { return (cnt + (size_t)vecs * 4 + 15) / 16 * 16; }

// gpp_*_workspace_bytes: `tab` is the score's tab_offset for these sizes (plain arithmetic: it may be formed before the sizes are checked);
// behind it the lines of the largest call, max_frames frames or S sequences
inline int workspace_size(long long cells, long long vecs, int max_frames, int S, size_t tab, size_t* bytes)
{
    if (sizes_bad(cells, vecs) || max_frames < 0 || S < 0 || !bytes) return GPP_ERR_BAD_ARG;
    if (sizes_unsupported(cells, vecs)) return GPP_ERR_UNSUPPORTED;
    const size_t frames = (size_t)max_frames * kTabCols, seqs = (size_t)S * kSeqTabCols;
    *bytes = (tab + (frames > seqs ? frames : seqs) * sizeof(int32_t) + 255) / 256 * 256;
    return GPP_OK;
}

// what the calls that walk frames (gpp_hota_potential, gpp_hota_match, gpp_idf1_count) check alike; `tab` as above.
// GPP_OK with *launch == false: nothing to do
inline int check_frames(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
                        const int32_t* trk, int N, int D, int A, int metric, const int32_t* frame_tab, long long cells, long long vecs,
                        size_t tab, void* workspace, size_t workspace_bytes, bool* launch)
{
    *launch = false;
    if (N < 0 || D < 0 || A < 0 || sizes_bad(cells, vecs) || metric < 0 || metric > 2) return GPP_ERR_BAD_ARG;
    if (D > GPP_KITTI_MAX_DETECTIONS || A > GPP_KITTI_MAX_DETECTIONS || sizes_unsupported(cells, vecs)) return GPP_ERR_UNSUPPORTED;
    if (N == 0) return GPP_OK;
    if (!frame_tab || !workspace) return GPP_ERR_BAD_ARG;
    if (A > 0 && (!label_outcome || !traj)) return GPP_ERR_BAD_ARG;
    if (D > 0 && (!row_outcome || !trk)) return GPP_ERR_BAD_ARG;
    if (D > 0 && A > 0 && !overlaps) return GPP_ERR_BAD_ARG;
    for (int f = 0; f < N; ++f)
        if (!line_ok(frame_tab + (size_t)f * kTabCols, f ? frame_tab + (size_t)(f - 1) * kTabCols : nullptr, cells, vecs)) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)workspace & 15u) return GPP_ERR_ALIGN;
    if (workspace_bytes < tab + (size_t)N * kTabCols * sizeof(int32_t)) return GPP_ERR_WORKSPACE;
    *launch = true;
    return GPP_OK;
}

// `n` lines of `cols` host integers to workspace + tab, on the call's stream, for the kernel launched after it
inline hipError_t upload_lines(void* workspace, size_t tab, const int32_t* lines, int n, int cols, hipStream_t stream)
{
    return hipMemcpyAsync((unsigned char*)workspace + tab, lines, (size_t)n * cols * sizeof(int32_t), hipMemcpyHostToDevice, stream);
}

// the return value of an entry point behind its kernel launch
inline int launched() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? GPP_OK : (int)e; }

}  // namespace gpp_pairs
