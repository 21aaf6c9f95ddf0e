// The assignment routine of DESIGN.md section 4.29 as a __device__ function: the Hungarian method in its shortest-augmenting-path form on a
// square int32 matrix in LDS, run by ONE wavefront, with the wavefront primitives it needs.  include/gpp.h (gpp_mot_assign, "assignment")
// states the rule operation for operation; utils/mot_eval.assign_np is its host form.
// csrc/hota_eval.hip (HOTA, section 4.30) instantiates it.  The primitives (rank_below .. wave_sum) have this one copy: csrc/mot_eval.hip
// takes them from here too, with the same device listing.  Only assign_kernel's BODY there still carries assign_rows' statements: built
// on assign_rows its listing differs from the parent's in several hundred lines (another register allocation and schedule), and
// alternating with the parent in one session gpp_mot_assign's median on 7 991 KITTI-sized frames was 119.7 - 120.3 us against
// 115.7 - 118.5 us in each of four repeats (profiles/hota/ab_mot_assign.jsonl) -- beyond the parent's own spread, so that body was left
// as it is.  The statements of assign_rows below are that body's, unchanged.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpp_mot {

constexpr int kWave = 64;

__device__ __forceinline__ int rank_below(unsigned long long lo, unsigned long long hi, int i)
{
    return i < 64 ? __popcll(lo & ((1ull << i) - 1ull)) : __popcll(lo) + __popcll(hi & ((1ull << (i - 64)) - 1ull));
}

// the value lane `lane` holds; `lane` is the same in every lane (a scalar read, no trip through the LDS crossbar)
__device__ __forceinline__ int read_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ long long read_lane64(long long v, int lane)
{
    const unsigned lo = (unsigned)read_lane((int)(unsigned)v, lane), hi = (unsigned)read_lane((int)(unsigned)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the key of the lane a DPP control names, all ones where the control names none (rows outside kRowMask, lanes shifted in from outside a row)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned long long dpp_key(unsigned long long key)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)key, kCtrl, kRowMask, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)(key >> 32), kCtrl, kRowMask, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}

// the smallest key of the wavefront, in every lane: a prefix minimum inside each row of 16 lanes (row_shr 1, 2, 4, 8), then lane 15 of a row
// into the next row (row_bcast:15, rows 1 and 3) and lane 31 into the upper half (row_bcast:31, rows 2 and 3): lane 63 holds the minimum
__device__ __forceinline__ unsigned long long wave_min(unsigned long long key)
{
    unsigned long long other;
    other = dpp_key<0x111, 0xf>(key); key = other < key ? other : key;
    other = dpp_key<0x112, 0xf>(key); key = other < key ? other : key;
    other = dpp_key<0x114, 0xf>(key); key = other < key ? other : key;
    other = dpp_key<0x118, 0xf>(key); key = other < key ? other : key;
    other = dpp_key<0x142, 0xa>(key); key = other < key ? other : key;
    other = dpp_key<0x143, 0xc>(key); key = other < key ? other : key;
    return (unsigned long long)read_lane64((long long)key, 63);
}

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// The assignment of the n x n matrix s_cost (n <= 128, read-only here): rows in order, each by a shortest augmenting path.  Lane l owns
// the columns l and l + 64; on return p[s] is the row that column lane + 64 s holds.  0 <= a reduced cost < 2^36.
__device__ __forceinline__ void assign_rows(const int32_t* s_cost, int n, int lane, int (&p)[2])
{
    long long u[2] = {0, 0}, v[2] = {0, 0};
    p[0] = p[1] = -1;
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
}

}  // namespace gpp_mot
