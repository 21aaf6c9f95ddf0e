// KITTI's object benchmark on gfx950 (MI355X): the overlaps of every (detection, label) pair -- image box, bird's-eye-view box, 3-D
// box -- and the matching of one image for every (metric, difficulty, score threshold) at once.  DESIGN.md section 4.17 is the
// specification (a restatement of the devkit's evaluate_object.cpp; parity with the devkit itself is unpinned); utils/kitti_eval.py is
// the host form, tests/kitti_oracle.py the loop-written oracle.  Table layouts and error codes: include/gpp.h, gpp_kitti_*.
//
//   kitti_overlaps_kernel   one thread per (detection, label) pair.  The bird's-eye-view intersection clips the detection's rectangle
//                           against the four edges of the label's (Sutherland-Hodgman).  The polygon grows by at most one vertex per
//                           edge, 4 -> 8, and is indexed at run time: it lives in LDS, two buffers of 8 vertices per thread laid out
//                           [buffer][vertex][thread] (consecutive lanes, consecutive doubles: no bank conflict), 16 KB per workgroup of
//                           64 threads.  The label's corners are indexed by an unrolled loop and stay in registers.  No scratch.
//                           The clipping itself is rot_iou.h, which cuboid_nms.hip shares.
//   kitti_stats_kernel      one workgroup per image, one thread per (metric, difficulty, threshold) triple, each walking the labels
//                           serially as the devkit does; the set of assigned detections is a 128-bit mask in two registers.  Scores,
//                           alphas and the status vectors of the image are staged in LDS, the four overlap planes too when they fit
//                           (D * A <= 1536: 48 KB); beyond that they are read from global memory (every thread of one metric reads
//                           the same address: a broadcast either way).
//
// Arithmetic: float64, every operation separate (this file is compiled with -ffp-contract=off): with r_y = 0 and dyadic coordinates
// every step is exact, so an IoU of exactly 7/10 is the double 0.7 and is not "> 0.7".  An intersection point is
// (p dq - q dp) / (dq - dp) with dp, dq the cross products against the clipping edge: exact whenever the point is representable.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"
#include "rot_iou.h"

namespace {

constexpr int kMaxD = GPP_KITTI_MAX_DETECTIONS;
constexpr int kMaxA = GPP_KITTI_MAX_LABELS;
constexpr int kMaxT = GPP_KITTI_MAX_THRESHOLDS;
constexpr int kRow = GPP_POSE_COLS;
constexpr int kLab = GPP_KITTI_LABEL_COLS;
constexpr int kPairThreads = 64;
constexpr int kMaxVerts = rot_iou::kMaxVerts;
constexpr int kStagedPairs = 1536;                   // 4 planes * 1536 pairs * 8 bytes = 48 KB of LDS

__device__ inline double dmin(double a, double b) { return a < b ? a : b; }
__device__ inline double dmax(double a, double b) { return a > b ? a : b; }

__global__ __launch_bounds__(kPairThreads) void kitti_overlaps_kernel(const float* __restrict__ rows, const double* __restrict__ labels,
                                                                      const int32_t* __restrict__ label_counts, int D, int A,
                                                                      double* __restrict__ overlaps)
{
    __shared__ double s_x[2][kMaxVerts][kPairThreads];
    __shared__ double s_z[2][kMaxVerts][kPairThreads];

    const int b = blockIdx.y, tid = threadIdx.x;
    const int pair = blockIdx.x * kPairThreads + tid;
    if (pair >= D * A) return;                       // (no barrier in this kernel)
    const int d = pair / A, a = pair - d * A;
    int n_lab = label_counts[b];
    n_lab = n_lab < 0 ? 0 : (n_lab > A ? A : n_lab);
    const float* __restrict__ r = rows + ((size_t)b * D + d) * kRow;
    const double* __restrict__ g = labels + ((size_t)b * A + a) * kLab;
    const size_t plane = (size_t)D * A;
    double* __restrict__ out = overlaps + (size_t)b * 4 * plane + (size_t)d * A + a;
    if (a >= n_lab || !(r[14] >= 0.0f)) {            // a padding label or a padding row
        out[0] = 0.0; out[plane] = 0.0; out[2 * plane] = 0.0; out[3 * plane] = 0.0;
        return;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- image box: no "+1"; a non-positive width or height is no overlap
    const double dx1 = (double)r[26], dy1 = (double)r[27], dx2 = (double)r[28], dy2 = (double)r[29];
    const double gx1 = g[4], gy1 = g[5], gx2 = g[6], gy2 = g[7];
    double o_img, o_dc;
    if (isnan(dx1) || isnan(dy1) || isnan(dx2) || isnan(dy2) || isnan(gx1) || isnan(gy1) || isnan(gx2) || isnan(gy2)) {
        o_img = nan; o_dc = nan;
    } else {
        const double w = dmin(dx2, gx2) - dmax(dx1, gx1);
        const double h = dmin(dy2, gy2) - dmax(dy1, gy1);
        if (w <= 0.0 || h <= 0.0) {
            o_img = 0.0; o_dc = 0.0;
        } else {
            const double inter = w * h;
            const double area_d = (dx2 - dx1) * (dy2 - dy1);
            const double area_g = (gx2 - gx1) * (gy2 - gy1);
            o_img = inter / (area_d + area_g - inter);
            o_dc = inter / area_d;
        }
    }

    // ---- bird's-eye view: two rotated rectangles in the (X, Z) plane
    const double dh = (double)r[30], dw = (double)r[17], dl = (double)r[18];
    const double dtx = (double)r[19], dty = (double)r[31], dtz = (double)r[21], dry = (double)r[32];
    const double gh = g[8], gw = g[9], gl = g[10], gtx = g[11], gty = g[12], gtz = g[13], gry = g[14];
    double o_bev, o_3d;
    if (isnan(dw) || isnan(dl) || isnan(dtx) || isnan(dtz) || isnan(dry) || isnan(gw) || isnan(gl) || isnan(gtx) || isnan(gtz) || isnan(gry)) {
        o_bev = nan; o_3d = nan;
    } else {
        // corners (+,+) (-,+) (-,-) (+,-) of (l/2, w/2): counter-clockwise in (x, z), and the placement is a rotation (rot_iou.h)
        double gX[4], gZ[4];
        {
            const double c = cos(gry), s = sin(gry), hl = gl / 2.0, hw = gw / 2.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) rot_iou::corner(k, c, s, hl, hw, gtx, gtz, gX[k], gZ[k]);
        }
        {
            const double c = cos(dry), s = sin(dry), hl = dl / 2.0, hw = dw / 2.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) rot_iou::corner(k, c, s, hl, hw, dtx, dtz, s_x[0][k][tid], s_z[0][k][tid]);
        }
        const double inter = rot_iou::intersection<kPairThreads>(s_x, s_z, tid, gX, gZ);
        const double area_d = dl * dw, area_g = gl * gw;
        o_bev = inter / (area_d + area_g - inter);
        if (isnan(dh) || isnan(dty) || isnan(gh) || isnan(gty)) {
            o_3d = nan;
        } else {
            const double hh = rot_iou::height_overlap(dty, dh, gty, gh);
            const double iv = inter * hh;
            const double vol_d = area_d * dh, vol_g = area_g * gh;
            o_3d = iv / (vol_d + vol_g - iv);
        }
    }
    out[0] = o_img; out[plane] = o_bev; out[2 * plane] = o_3d; out[3 * plane] = o_dc;
}

template <bool STAGED>
__global__ __launch_bounds__(384) void kitti_stats_kernel(const float* __restrict__ rows, const double* __restrict__ labels,
                                                          const int32_t* __restrict__ label_counts, const double* __restrict__ overlaps,
                                                          double mo0, double mo1, double mo2, const float* __restrict__ thresholds,
                                                          const int32_t* __restrict__ n_thresholds, int D, int A, int T,
                                                          float* __restrict__ tp_scores, int32_t* __restrict__ n_gt,
                                                          int32_t* __restrict__ stats, double* __restrict__ similarity)
{
    extern __shared__ double s_ov[];                 // STAGED: the image's four planes
    __shared__ double s_dalpha[kMaxD];
    __shared__ double s_galpha[kMaxA];
    __shared__ float s_score[kMaxD];
    __shared__ signed char s_dstat[3][kMaxD];
    __shared__ signed char s_lstat[3][kMaxA];
    __shared__ unsigned char s_dc[kMaxA];

    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    int n_lab = label_counts[b];
    n_lab = n_lab < 0 ? 0 : (n_lab > A ? A : n_lab);
    const size_t plane = (size_t)D * A;
    const double* __restrict__ ov_g = overlaps + (size_t)b * 4 * plane;

    for (int j = tid; j < D; j += nthreads) {
        const float* __restrict__ r = rows + ((size_t)b * D + j) * kRow;
        const bool det = r[14] >= 0.0f;
        s_score[j] = r[12];
        s_dalpha[j] = (double)r[25];
        const double height = fabs((double)r[29] - (double)r[27]);
        // every detection is a Car: the devkit's -1 (another class) is the padding row here
        s_dstat[0][j] = !det ? -1 : (height < 40.0 ? 1 : 0);
        s_dstat[1][j] = !det ? -1 : (height < 25.0 ? 1 : 0);
        s_dstat[2][j] = s_dstat[1][j];
    }
    for (int a = tid; a < A; a += nthreads) {
        signed char st0 = -1, st1 = -1, st2 = -1;
        unsigned char dc = 0;
        double alpha = 0.0;
        if (a < n_lab) {
            const double* __restrict__ g = labels + ((size_t)b * A + a) * kLab;
            const double type = g[0], trunc = g[1], occ = g[2];
            const double height = fabs(g[7] - g[5]);
            alpha = g[3];
            const bool ig0 = occ > 0.0 || trunc > 0.15 || height < 40.0;
            const bool ig1 = occ > 1.0 || trunc > 0.30 || height < 25.0;
            const bool ig2 = occ > 2.0 || trunc > 0.50 || height < 25.0;
            if (type == 0.0) { st0 = ig0 ? 1 : 0; st1 = ig1 ? 1 : 0; st2 = ig2 ? 1 : 0; }
            else if (type == 1.0) { st0 = 1; st1 = 1; st2 = 1; }
            dc = type == 2.0 ? 1 : 0;
        }
        s_lstat[0][a] = st0; s_lstat[1][a] = st1; s_lstat[2][a] = st2;
        s_dc[a] = dc;
        s_galpha[a] = alpha;
    }
    if (STAGED)
        for (size_t i = tid; i < 4 * plane; i += nthreads) s_ov[i] = ov_g[i];
    __syncthreads();

    const bool compute_fp = thresholds != nullptr;
    const int per_bin = compute_fp ? T : 1;
    if (tid >= 9 * per_bin) return;
    const int bin = tid / per_bin, k = tid - bin * per_bin;      // bin = 3 * metric + difficulty
    const int m = bin / 3, diff = bin - 3 * m;
    const double min_ov = m == 0 ? mo0 : (m == 1 ? mo1 : mo2);
    const double* __restrict__ ov = STAGED ? s_ov : ov_g;
    const double* __restrict__ ov_m = ov + (size_t)m * plane;
    const double* __restrict__ ov_dc = ov + 3 * plane;

    if (compute_fp && k >= n_thresholds[bin]) {
        int32_t* __restrict__ s = stats + (((size_t)b * 9 + bin) * T + k) * 3;
        s[0] = 0; s[1] = 0; s[2] = 0;
        similarity[((size_t)b * 9 + bin) * T + k] = 0.0;
        return;
    }
    const float thr = compute_fp ? thresholds[(size_t)bin * T + k] : 0.0f;
    const float qnan = __int_as_float(0x7fc00000);

    uint64_t as_lo = 0, as_hi = 0;                   // the assigned detections
    int tp = 0, fp = 0, fn = 0, gt = 0;
    double sim = 0.0;
    for (int a = 0; a < n_lab; ++a) {
        const int ls = s_lstat[diff][a];
        float tp_score = qnan;
        if (ls != -1) {
            gt += ls == 0 ? 1 : 0;
            int cand = -1;
            bool cand_ignored = false;
            double max_ov = 0.0;
            float best = -INFINITY;
            for (int j = 0; j < D; ++j) {
                const int ds = s_dstat[diff][j];
                const bool taken = ((j < 64 ? as_lo >> j : as_hi >> (j - 64)) & 1) != 0;
                const float score = s_score[j];
                if (ds == -1 || taken || (compute_fp && score < thr)) continue;
                const double o = ov_m[(size_t)j * A + a];
                if (!(o > min_ov)) continue;
                if (!compute_fp) {
                    if (score > best) { cand = j; best = score; }
                } else if (ds == 0 && (o > max_ov || cand_ignored)) {
                    max_ov = o; cand = j; cand_ignored = false;
                } else if (ds == 1 && cand == -1) {
                    cand = j; cand_ignored = true;
                }
            }
            if (cand == -1) {
                fn += ls == 0 ? 1 : 0;
            } else {
                if (!(ls == 1 || s_dstat[diff][cand] == 1)) {
                    ++tp;
                    tp_score = s_score[cand];
                    if (m == 0 && compute_fp) sim = sim + (1.0 + cos(s_galpha[a] - s_dalpha[cand])) / 2.0;
                }
                if (cand < 64) as_lo |= 1ull << cand; else as_hi |= 1ull << (cand - 64);
            }
        }
        if (!compute_fp) tp_scores[((size_t)b * 9 + bin) * A + a] = tp_score;
    }
    if (!compute_fp) {
        for (int a = n_lab; a < A; ++a) tp_scores[((size_t)b * 9 + bin) * A + a] = qnan;
        n_gt[b * 9 + bin] = gt;
        return;
    }
    // what is left above the threshold is a false positive -- for the image metric unless it lies in a DontCare region
    for (int j = 0; j < D; ++j) {
        const bool taken = ((j < 64 ? as_lo >> j : as_hi >> (j - 64)) & 1) != 0;
        if (taken || s_dstat[diff][j] != 0 || s_score[j] < thr) continue;
        bool stuff = false;
        if (m == 0)
            for (int a = 0; a < n_lab; ++a)
                if (s_dc[a] && ov_dc[(size_t)j * A + a] > min_ov) stuff = true;
        fp += stuff ? 0 : 1;
    }
    int32_t* __restrict__ s = stats + (((size_t)b * 9 + bin) * T + k) * 3;
    s[0] = tp; s[1] = fp; s[2] = fn;
    similarity[((size_t)b * 9 + bin) * T + k] = sim;
}

}  // namespace

extern "C" int gpp_kitti_overlaps_f64(const float* rows, const double* labels, const int32_t* label_counts, int B, int D, int A,
                                      double* overlaps, void* stream)
{
    if (B < 0 || D < 0 || A < 0) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_OK;
    if (!rows || !label_counts || (A > 0 && (!labels || !overlaps))) return GPP_ERR_BAD_ARG;
    if (D > kMaxD || A > kMaxA) return GPP_ERR_UNSUPPORTED;
    if (A == 0) return GPP_OK;
    if (B > 65535) return GPP_ERR_UNSUPPORTED;       // (grid.y; utils/kitti_eval.py's chunks stay far below)
    const unsigned blocks = (unsigned)((D * A + kPairThreads - 1) / kPairThreads);
    kitti_overlaps_kernel<<<dim3(blocks, (unsigned)B), dim3(kPairThreads), 0, (hipStream_t)stream>>>(rows, labels, label_counts, D, A, overlaps);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_kitti_stats_f64(const float* rows, const double* labels, const int32_t* label_counts, const double* overlaps,
                                   const double* min_overlap, const float* thresholds, const int32_t* n_thresholds, int B, int D, int A,
                                   int T, float* tp_scores, int32_t* n_gt, int32_t* stats, double* similarity, void* stream)
{
    if (B < 0 || D < 0 || A < 0 || T < 0 || T > kMaxT) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_OK;
    if (!rows || !label_counts || !min_overlap || (A > 0 && (!labels || !overlaps))) return GPP_ERR_BAD_ARG;
    const bool pass2 = thresholds != nullptr;
    if (pass2 ? (!n_thresholds || !stats || !similarity) : (!n_gt || (A > 0 && !tp_scores))) return GPP_ERR_BAD_ARG;
    if (D > kMaxD || A > kMaxA) return GPP_ERR_UNSUPPORTED;
    if (pass2 && T == 0) return GPP_OK;
    const unsigned threads = pass2 ? (unsigned)((9 * T + 63) / 64 * 64) : 64u;
    const bool staged = D * A <= kStagedPairs;
    const size_t lds = staged ? (size_t)4 * D * A * sizeof(double) : 0;
    if (staged)
        kitti_stats_kernel<true><<<dim3((unsigned)B), dim3(threads), lds, (hipStream_t)stream>>>(
            rows, labels, label_counts, overlaps, min_overlap[0], min_overlap[1], min_overlap[2], thresholds, n_thresholds, D, A, T,
            tp_scores, n_gt, stats, similarity);
    else
        kitti_stats_kernel<false><<<dim3((unsigned)B), dim3(threads), 0, (hipStream_t)stream>>>(
            rows, labels, label_counts, overlaps, min_overlap[0], min_overlap[1], min_overlap[2], thresholds, n_thresholds, D, A, T,
            tp_scores, n_gt, stats, similarity);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
