// Greedy suppression of duplicate cuboids on gfx950 (MI355X): the rows of gpp_pose_f32 of one image, ranked by score, each kept iff no
// kept row overlaps it by more than a threshold -- overlap = the rotated-rectangle IoU of the bird's-eye view or the 3-D IoU of KITTI's
// benchmark (rot_iou.h: the arithmetic of kitti_eval.hip, operation for operation).  DESIGN.md section 4.26 is the specification,
// utils/cuboid_nms.py the host form, tests/cuboid_nms_oracle.py the loop-written oracle; include/gpp.h has the contract.
//
//   cuboid_nms_kernel   one workgroup of 128 threads per image, five phases with a barrier between them:
//     1  one thread per row: liveness, the placed corners, area, height fields and the NaN flags into LDS (every input byte the
//        decisions need is read here, before anything is written: rows_out may be rows_in)
//     2  one thread per row: its place in the list of live rows (ascending row index) and its rank (score descending, row ascending)
//     3  the n (n - 1) / 2 pairs of live rows over the lanes: row i < j, i's rectangle clipped against j's edges, the polygon in LDS
//        [buffer][vertex][thread]; "overlap > threshold" goes as one bit each way into a D x 128-bit table in LDS.  A pair whose
//        centres lie further apart than the two half-diagonals (with slack) has an empty intersection and skips the clipping: the
//        lanes first gate 4096 pairs and list the survivors in LDS, then clip the list together (no lane waits for a neighbour's clip)
//     4  lane 0 walks the ranks with the kept set as a 128-bit mask
//     5  one thread per row writes the row, the suppressor and (thread 0) the count
//
// Arithmetic: float64, every operation separate (this file is compiled with -ffp-contract=off), as kitti_eval.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"
#include "rot_iou.h"

namespace {

constexpr int kMaxD = GPP_KITTI_MAX_DETECTIONS;
constexpr int kRow = GPP_POSE_COLS;
constexpr int kThreads = 128;
constexpr int kWords = kMaxD / 32;
// the gate's slack on the SQUARED distance: (1 + 1/32)^2.  The gate skips a pair only when the circles around the two rectangles are
// separated by more than 3 % of their radii -- decimetres, against the 1e-14 m that the rounding of squares, sums and one sqrt can move
// either side of the comparison
constexpr double kGateSlack = 1.0634765625;

constexpr int kChunk = 4096;                         // pairs gated per round (8 KB of offsets): D = 100 has 4950 pairs, D = 128 8128

static_assert(kThreads >= kMaxD, "one thread per row");
static_assert(kChunk <= 65536, "a pair's offset into its chunk is 16 bits");

// pair p of the strictly lower triangle, row-major: p = c (c - 1) / 2 + a, 0 <= a < c
__device__ __forceinline__ void pair_of(int p, int& a, int& c)
{
    c = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
    while (c * (c - 1) / 2 > p) --c;
    while ((c + 1) * c / 2 <= p) ++c;
    a = p - c * (c - 1) / 2;
}

__global__ __launch_bounds__(kThreads) void cuboid_nms_kernel(const float* rows_in, int D, int metric, double iou_thr, float* rows_out,
                                                              int32_t* __restrict__ counts, int32_t* __restrict__ suppressor)
{
    __shared__ double s_x[2][rot_iou::kMaxVerts][kThreads];
    __shared__ double s_z[2][rot_iou::kMaxVerts][kThreads];
    __shared__ double s_cx[4][kMaxD], s_cz[4][kMaxD];    // the placed corners of every row
    __shared__ double s_tx[kMaxD], s_tz[kMaxD], s_rad[kMaxD], s_area[kMaxD], s_h[kMaxD], s_y[kMaxD];
    __shared__ float s_score[kMaxD];
    __shared__ uint32_t s_tab[kMaxD][kWords];            // bit j of row i: overlap(i, j) > threshold
    __shared__ int16_t s_list[kMaxD], s_rank[kMaxD], s_order[kMaxD], s_by[kMaxD];
    __shared__ unsigned char s_flag[kMaxD];              // 1 live, 2 a NaN among the bird's-eye-view fields, 4 a NaN among h, y
    __shared__ uint16_t s_pairs[kChunk];                 // the pairs of the chunk that pass the gate, as offsets into the chunk
    __shared__ int s_live, s_listed;

    const int b = blockIdx.x, tid = threadIdx.x;
    const float* src = rows_in + (size_t)b * D * kRow;
    float* dst = rows_out + (size_t)b * D * kRow;

    // ---- 1: the rows
    if (tid < kMaxD) {
        unsigned char flag = 0;
        float score = -INFINITY;
        if (tid < D) {
            const float* r = src + (size_t)tid * kRow;
            if (r[14] >= 0.0f) {
                flag = 1;
                score = r[12];
                if (isnan(score)) score = -INFINITY;     // (a NaN score ranks last: the order stays total)
                const double dw = (double)r[17], dl = (double)r[18], dtx = (double)r[19], dtz = (double)r[21], dry = (double)r[32];
                const double dh = (double)r[30], dty = (double)r[31];
                if (isnan(dw) || isnan(dl) || isnan(dtx) || isnan(dtz) || isnan(dry)) flag |= 2;
                if (isnan(dh) || isnan(dty)) flag |= 4;
                const double c = cos(dry), s = sin(dry), hl = dl / 2.0, hw = dw / 2.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) rot_iou::corner(k, c, s, hl, hw, dtx, dtz, s_cx[k][tid], s_cz[k][tid]);
                s_tx[tid] = dtx; s_tz[tid] = dtz;
                s_rad[tid] = sqrt(hl * hl + hw * hw);
                s_area[tid] = dl * dw;
                s_h[tid] = dh; s_y[tid] = dty;
            }
        }
        s_flag[tid] = flag;
        s_score[tid] = score;
        s_order[tid] = -1;
        s_by[tid] = -1;
#pragma unroll
        for (int k = 0; k < kWords; ++k) s_tab[tid][k] = 0u;
    }
    __syncthreads();

    // ---- 2: the list of live rows and the rank of each
    if (tid < D && (s_flag[tid] & 1)) {
        const float mine = s_score[tid];
        int before = 0, rank = 0;
        for (int j = 0; j < D; ++j) {
            if (!(s_flag[j] & 1)) continue;
            before += j < tid ? 1 : 0;
            const float other = s_score[j];
            rank += (other > mine || (other == mine && j < tid)) ? 1 : 0;
        }
        s_list[before] = (int16_t)tid;                   // (before, rank < the number of live rows <= D: both are permutations)
        s_rank[tid] = (int16_t)rank;
        s_order[rank] = (int16_t)tid;
    }
    if (tid == 0) {
        int n = 0;
        for (int j = 0; j < D; ++j) n += s_flag[j] & 1;
        s_live = n;
    }
    __syncthreads();

    // ---- 3: the pairs.  p = c (c - 1) / 2 + a with a < c: rows i = list[a] < j = list[c].  Chunk by chunk, first every lane gates its
    // pairs and the survivors are listed (in any order: the table does not depend on it), then the list is clipped with every lane busy --
    // clipped where they are met, the few pairs of a scene that overlap would stall their whole wavefront once per round
    const int n = s_live, pairs = n * (n - 1) / 2;
    for (int base = 0; base < pairs; base += kChunk) {
        if (tid == 0) s_listed = 0;
        __syncthreads();
        const int end = base + kChunk < pairs ? base + kChunk : pairs;
        for (int p = base + tid; p < end; p += kThreads) {
            int a, c;
            pair_of(p, a, c);
            const int i = s_list[a], j = s_list[c];
            const unsigned fl = s_flag[i] | s_flag[j];
            if ((fl & 2) || (metric == GPP_CUBOID_NMS_3D && (fl & 4))) continue;   // a NaN operand: a NaN overlap, which is above nothing
            // the gate: an empty intersection is an overlap of 0 (or 0 / 0), which is above no threshold either
            const double ddx = s_tx[i] - s_tx[j], ddz = s_tz[i] - s_tz[j], reach = s_rad[i] + s_rad[j];
            if (ddx * ddx + ddz * ddz > reach * reach * kGateSlack) continue;
            s_pairs[atomicAdd(&s_listed, 1)] = (uint16_t)(p - base);               // (at most kChunk pairs are looked at per chunk)
        }
        __syncthreads();
        const int listed = s_listed;
        for (int q = tid; q < listed; q += kThreads) {
            int a, c;
            pair_of(base + s_pairs[q], a, c);
            const int i = s_list[a], j = s_list[c];
            double gX[4], gZ[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                gX[k] = s_cx[k][j]; gZ[k] = s_cz[k][j];
                s_x[0][k][tid] = s_cx[k][i]; s_z[0][k][tid] = s_cz[k][i];
            }
            const double inter = rot_iou::intersection<kThreads>(s_x, s_z, tid, gX, gZ);
            const double area_d = s_area[i], area_g = s_area[j];
            double o;
            if (metric == GPP_CUBOID_NMS_BEV) {
                o = inter / (area_d + area_g - inter);
            } else {
                const double dh = s_h[i], gh = s_h[j];
                const double hh = rot_iou::height_overlap(s_y[i], dh, s_y[j], gh);
                const double iv = inter * hh;
                const double vol_d = area_d * dh, vol_g = area_g * gh;
                o = iv / (vol_d + vol_g - iv);
            }
            if (o > iou_thr) {
                atomicOr(&s_tab[i][j >> 5], 1u << (j & 31));
                atomicOr(&s_tab[j][i >> 5], 1u << (i & 31));
            }
        }
        __syncthreads();
    }

    // ---- 4: the greedy pass
    if (tid == 0) {
        uint32_t kept[kWords] = {0u, 0u, 0u, 0u};
        int count = 0;
        for (int r = 0; r < n; ++r) {
            const int d = s_order[r];
            if (d < 0) continue;                         // (cannot happen: the ranks are a permutation)
            int by = -1, by_rank = kMaxD;
#pragma unroll
            for (int k = 0; k < kWords; ++k) {
                uint32_t hits = s_tab[d][k] & kept[k];
                while (hits) {
                    const int e = 32 * k + __ffs((int)hits) - 1;
                    hits &= hits - 1;
                    if (s_rank[e] < by_rank) { by_rank = s_rank[e]; by = e; }
                }
            }
            if (by < 0) {
#pragma unroll
                for (int k = 0; k < kWords; ++k) kept[k] |= (d >> 5) == k ? 1u << (d & 31) : 0u;
                ++count;
            } else {
                s_by[d] = (int16_t)by;
            }
        }
        counts[b] = count;
    }
    __syncthreads();

    // ---- 5: the rows.  In place a kept row and a padding row stay where they are; otherwise they are copied word for word
    if (tid < D) {
        const int by = s_by[tid];
        suppressor[(size_t)b * D + tid] = by;
        float* w = dst + (size_t)tid * kRow;
        if (by >= 0) {
            for (int k = 0; k < kRow; ++k) w[k] = -1.0f;
        } else if (dst != src) {
            const uint32_t* from = (const uint32_t*)(src + (size_t)tid * kRow);
            uint32_t* to = (uint32_t*)w;
            for (int k = 0; k < kRow; ++k) to[k] = from[k];
        }
    }
}

}  // namespace

extern "C" int gpp_cuboid_nms_f64(const float* rows_in, int B, int D, int metric, double iou_thr, float* rows_out, int32_t* counts,
                                  int32_t* suppressor, void* stream)
{
    if (B < 0 || D < 0) return GPP_ERR_BAD_ARG;
    if (metric != GPP_CUBOID_NMS_BEV && metric != GPP_CUBOID_NMS_3D) return GPP_ERR_BAD_ARG;
    if (!(iou_thr > 0.0 && iou_thr < 1.0)) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_OK;
    if (!rows_in || !rows_out || !counts || !suppressor) return GPP_ERR_BAD_ARG;
    if (D > kMaxD) return GPP_ERR_UNSUPPORTED;
    cuboid_nms_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(rows_in, D, metric, iou_thr, rows_out, counts, suppressor);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
