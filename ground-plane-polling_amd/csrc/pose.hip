// 6-DoF pose and KITTI fields of the detections on gfx950 (MI355X): one thread per detection, one workgroup per image.
//
// Restates what /root/reference/keras_retinanet_3D/bin/run_network.py does on the host after predict_on_batch:
//   scale correction and selection :113-135, pose from the 3-D keypoints :137-247 (the two live `outlier` branches),
//   cuboid corners and the KITTI fields :298-330
// (utils/gpp_utils.py select_detections / recover_pose / cuboid_corners / kitti_lines on the host side of this package).
// Row layout: include/gpp.h, gpp_pose_f32.
//
// Arithmetic: the float32 inputs are widened once, every step is float64 with every operation separate (this file is compiled
// with -ffp-contract=off), and a value is rounded to float32 once, where it is stored.  The host path keeps float32 intermediates
// (the reference's float32 arrays) and a float64 Rodrigues; a detection hundreds of metres away loses millimetres there.
//
// cv2.Rodrigues(matrix) first replaces the matrix by the nearest rotation, U V^T of its SVD = its polar factor.  Here: Newton's
// iteration X <- (g X + X^-T / g) / 2 with Higham's Frobenius scaling g = sqrt(|X^-1|_F / |X|_F), a fixed number of steps (it
// converges quadratically from any non-singular start; [x y z] has two unit columns and a third orthogonal to both, 6 steps reach
// 1e-16 from a 30 degree skew, kPolarSteps leaves room down to a condition number of 1e12).  The 3x3 lives in nine named
// registers: no array, nothing indexed at run time, no scratch.
// cv2.Rodrigues(vector) of that result, needed for the corner heights only, is rebuilt from the same cosine: cos(t) = c,
// sin(t) = sqrt((1 - c)(1 + c)) for t = acos(c) in [0, pi] -- no sine or cosine call (their large-argument reduction uses a table
// indexed at run time).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"
#include "track_kf.h"

namespace {

using gpp_kf::kPi;
using gpp_kf::wrap;                                  // run_network.py:312-316: a % 2 pi, then into [-pi, pi); the trackers wrap alike

constexpr int kThreads = 128;
constexpr int kPolarSteps = 12;

struct M3 { double a00, a01, a02, a10, a11, a12, a20, a21, a22; };

__host__ __device__ inline bool finite9(const M3& m)
{
    return isfinite(m.a00) && isfinite(m.a01) && isfinite(m.a02) && isfinite(m.a10) && isfinite(m.a11) && isfinite(m.a12) &&
           isfinite(m.a20) && isfinite(m.a21) && isfinite(m.a22);
}

__host__ __device__ inline double frob2(const M3& m)
{
    return m.a00 * m.a00 + m.a01 * m.a01 + m.a02 * m.a02 + m.a10 * m.a10 + m.a11 * m.a11 + m.a12 * m.a12 +
           m.a20 * m.a20 + m.a21 * m.a21 + m.a22 * m.a22;
}

// the polar factor of a non-singular 3x3 (a singular one gives NaN)
__host__ __device__ inline M3 polar(M3 x)
{
#pragma unroll 1
    for (int it = 0; it < kPolarSteps; ++it) {
        // cofactors: inverse transpose = cofactor matrix / determinant
        M3 c;
        c.a00 = x.a11 * x.a22 - x.a12 * x.a21;
        c.a01 = x.a12 * x.a20 - x.a10 * x.a22;
        c.a02 = x.a10 * x.a21 - x.a11 * x.a20;
        c.a10 = x.a02 * x.a21 - x.a01 * x.a22;
        c.a11 = x.a00 * x.a22 - x.a02 * x.a20;
        c.a12 = x.a01 * x.a20 - x.a00 * x.a21;
        c.a20 = x.a01 * x.a12 - x.a02 * x.a11;
        c.a21 = x.a02 * x.a10 - x.a00 * x.a12;
        c.a22 = x.a00 * x.a11 - x.a01 * x.a10;
        const double det = x.a00 * c.a00 + x.a01 * c.a01 + x.a02 * c.a02;
        const double inv_det = 1.0 / det;
        // g^2 = |X^-1|_F / |X|_F ;  X <- (g X + X^-T / g) / 2
        const double g = sqrt(sqrt(frob2(c)) * fabs(inv_det) / sqrt(frob2(x)));
        const double p = 0.5 * g, q = 0.5 * inv_det / g;
        x.a00 = p * x.a00 + q * c.a00; x.a01 = p * x.a01 + q * c.a01; x.a02 = p * x.a02 + q * c.a02;
        x.a10 = p * x.a10 + q * c.a10; x.a11 = p * x.a11 + q * c.a11; x.a12 = p * x.a12 + q * c.a12;
        x.a20 = p * x.a20 + q * c.a20; x.a21 = p * x.a21 + q * c.a21; x.a22 = p * x.a22 + q * c.a22;
    }
    return x;
}

// one detection above the threshold -> its row (include/gpp.h).  bx: its 12 box values, kp: its 4 x 3 keypoints, width: its dimension w
__host__ __device__ inline void pose_row(const float* __restrict__ bx, float width, float score, int label, int o,
                                         const float* __restrict__ kp, float residual, double scale, double img_h, double img_w,
                                         float* __restrict__ row)
{
    const double nan = __builtin_nan("");
    // :114: boxes /= scale
    const double x1 = (double)bx[0] / scale, y1 = (double)bx[1] / scale, x2 = (double)bx[2] / scale, y2 = (double)bx[3] / scale;
    row[0] = (float)x1; row[1] = (float)y1; row[2] = (float)x2; row[3] = (float)y2;
#pragma unroll
    for (int k = 4; k < 12; ++k) row[k] = (float)((double)bx[k] / scale);
    row[12] = score; row[13] = (float)label; row[14] = (float)o; row[15] = residual;
    row[26] = (float)fmax(x1, 0.0); row[27] = (float)fmax(y1, 0.0); row[28] = (float)fmin(x2, img_w); row[29] = (float)fmin(y2, img_h);
    row[33] = 0.0f; row[34] = 0.0f; row[35] = 0.0f;

    // :137-247.  X_s: the second bottom keypoint in use, X_l for orientation 0 and 3 (outlier = 2), X_r for 1 and 2 (outlier = 0)
    const bool left = (o == 0) || (o == 3);
    const double mx = kp[3], my = kp[4], mz = kp[5], tx = kp[9], ty = kp[10], tz = kp[11];
    const double sx = left ? kp[0] : kp[6], sy = left ? kp[1] : kp[7], sz = left ? kp[2] : kp[8];
    const double hx = mx - tx, hy = my - ty, hz = mz - tz;                       // X_m - X_t
    const double ex = mx - sx, ey = my - sy, ez = mz - sz;                       // X_m - X_s
    const double h = sqrt(hx * hx + hy * hy + hz * hz), l = sqrt(ex * ex + ey * ey + ez * ez);
    const double w = (double)width;
    row[16] = (float)h; row[17] = (float)w; row[18] = (float)l;
    const double sgn_x = (o == 0 || o == 1) ? 1.0 : -1.0;                        // x = (X_m - X_s) / l for 0, 1; (X_s - X_m) / l for 2, 3
    const double sgn_z = (o == 0 || o == 2) ? 1.0 : -1.0;                        // location = middle +- z w / 2
    M3 r;                                                                        // columns x, y, z
    r.a00 = sgn_x * ex / l; r.a10 = sgn_x * ey / l; r.a20 = sgn_x * ez / l;
    r.a01 = hx / h; r.a11 = hy / h; r.a21 = hz / h;
    r.a02 = r.a10 * r.a21 - r.a20 * r.a11;
    r.a12 = r.a20 * r.a01 - r.a00 * r.a21;
    r.a22 = r.a00 * r.a11 - r.a10 * r.a01;
    const double lx = (mx + sx) / 2.0 + sgn_z * r.a02 * w / 2.0;
    const double ly = (my + sy) / 2.0 + sgn_z * r.a12 * w / 2.0;
    const double lz = (mz + sz) / 2.0 + sgn_z * r.a22 * w / 2.0;

    double vx = nan, vy = nan, vz = nan, alpha = nan, kitti_h = nan, kitti_y = nan, r_y = nan;
    double ox = nan, oy = nan, oz = nan;
    const M3 u = polar(r);
    if (finite9(r) && finite9(u)) {
        ox = lx; oy = ly; oz = lz;
        // cv2.Rodrigues(matrix): axis * angle of the rotation u
        const double ax = u.a21 - u.a12, ay = u.a02 - u.a20, az = u.a10 - u.a01;
        const double s = sqrt((ax * ax + ay * ay + az * az) * 0.25);
        const double c = fmin(fmax((u.a00 + u.a11 + u.a22 - 1.0) * 0.5, -1.0), 1.0);
        const double theta = acos(c);
        double kx = 0.0, ky = 0.0, kz = 0.0;                                     // unit axis (0 for the identity)
        if (s >= 1e-5) {
            const double f = 1.0 / (2.0 * s);
            vx = ax * (theta * f); vy = ay * (theta * f); vz = az * (theta * f);
            const double n = sqrt(vx * vx + vy * vy + vz * vz);
            kx = vx / n; ky = vy / n; kz = vz / n;
        } else if (c > 0.0) {
            vx = 0.0; vy = 0.0; vz = 0.0;
        } else {                                                                 // a rotation by pi: the axis from the diagonal
            double qx = sqrt(fmax((u.a00 + 1.0) * 0.5, 0.0));
            double qy = sqrt(fmax((u.a11 + 1.0) * 0.5, 0.0)) * (u.a01 < 0.0 ? -1.0 : 1.0);
            double qz = sqrt(fmax((u.a22 + 1.0) * 0.5, 0.0)) * (u.a02 < 0.0 ? -1.0 : 1.0);
            if (fabs(qx) < fabs(qy) && fabs(qx) < fabs(qz) && ((u.a12 > 0.0) != (qy * qz > 0.0))) qz = -qz;
            const double n = sqrt(qx * qx + qy * qy + qz * qz);
            kx = qx / n; ky = qy / n; kz = qz / n;
            vx = kx * theta; vy = ky * theta; vz = kz * theta;
        }
        // :298-330: Y of the eight corners = row 1 of cv2.Rodrigues(vector) . (+-l/2, 0 or -h, +-w/2) + location y
        const bool rotated = (s >= 1e-5) || !(c > 0.0);
        const double cs = rotated ? c : 1.0, sn = rotated ? sqrt((1.0 - c) * (1.0 + c)) : 0.0;
        const double r10 = (1.0 - cs) * ky * kx + sn * kz;
        const double r11 = cs + (1.0 - cs) * ky * ky;
        const double r12 = (1.0 - cs) * ky * kz - sn * kx;
        const double px = fabs(r10 * (l / 2.0)), pz = fabs(r12 * (w / 2.0));      // max / min over the four (+-, +-) pairs
        const double top = r11 * (-h);
        const double ymax = fmax(0.0, top) + px + pz, ymin = fmin(0.0, top) - px - pz;
        kitti_y = ymax + oy;
        kitti_h = (ymax + oy) - (ymin + oy);
        r_y = wrap(vy);
        alpha = wrap(r_y + atan2(oz, ox) + 1.5 * kPi);
    }
    row[19] = (float)ox; row[20] = (float)oy; row[21] = (float)oz;
    row[22] = (float)vx; row[23] = (float)vy; row[24] = (float)vz;
    row[25] = (float)alpha;
    row[30] = (float)kitti_h; row[31] = (float)kitti_y; row[32] = (float)r_y;
}

__global__ __launch_bounds__(kThreads) void pose_kernel(const float* __restrict__ boxes, const float* __restrict__ dims,
                                                        const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ orientations, const float* __restrict__ keypoints,
                                                        const float* __restrict__ residuals, const float* __restrict__ frame_info,
                                                        int D, float score_thr, float* __restrict__ rows, int32_t* __restrict__ counts)
{
    __shared__ int s_count[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double scale = (double)frame_info[3 * b], img_h = (double)frame_info[3 * b + 1], img_w = (double)frame_info[3 * b + 2];
    int mine = 0;
    for (int d = tid; d < D; d += kThreads) {
        const size_t det = (size_t)b * D + d;
        float* __restrict__ row = rows + det * GPP_POSE_COLS;
        const float score = scores[det];
        const int o = orientations[det];
        if (!(score > score_thr) || o == -1) {
#pragma unroll
            for (int k = 0; k < GPP_POSE_COLS; ++k) row[k] = -1.0f;
            continue;
        }
        ++mine;
        pose_row(boxes + det * 12, dims[det * 3 + 1], score, labels[det], o, keypoints + det * 12, residuals[det], scale, img_h, img_w, row);
    }
    // rows of this image with a score above the threshold
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) mine += __shfl_xor(mine, sft, 64);
    if ((tid & 63) == 0) s_count[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) total += s_count[k];
        counts[b] = total;
    }
}

}  // namespace

extern "C" int gpp_pose_f32(const float* boxes, const float* dims, const float* scores, const int32_t* labels,
                            const int32_t* orientations, const float* keypoints, const float* residuals,
                            const float* frame_info, int B, int D, float score_thr,
                            float* rows, int32_t* counts, void* stream)
{
    if (B < 0 || D < 0) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_OK;
    if (!boxes || !dims || !scores || !labels || !orientations || !keypoints || !residuals || !frame_info || !rows || !counts)
        return GPP_ERR_BAD_ARG;
    pose_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(boxes, dims, scores, labels, orientations, keypoints,
                                                                               residuals, frame_info, D, score_thr, rows, counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
