// The intersection of two rotated rectangles in the (X, Z) plane, shared by kitti_eval.hip (detection against label) and
// cuboid_nms.hip (detection against detection): the corners, the four Sutherland-Hodgman steps and the area sum.  One sequence of
// float64 operations for both, so that both agree with utils/kitti_eval.py bit for bit -- the including files are compiled with
// -ffp-contract=off.  DESIGN.md section 4.17 is the specification.
//
// The clipped polygon grows by at most one vertex per edge, 4 -> 8, and is indexed at run time: it lives in LDS, two buffers of
// kMaxVerts vertices per thread laid out [buffer][vertex][thread] (consecutive lanes, consecutive doubles: no bank conflict).  The
// clipping rectangle's corners are indexed by unrolled loops and stay in registers.  No scratch.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace rot_iou {

constexpr int kMaxVerts = 8;

// corner k of the rectangle (l/2, w/2) = (hl, hw): (+,+) (-,+) (-,-) (+,-), counter-clockwise in (x, z); the placement is a rotation
// by (c, s) = (cos r_y, sin r_y) and a shift
__device__ __forceinline__ void corner(int k, double c, double s, double hl, double hw, double tx, double tz, double& X, double& Z)
{
    const double x = (k == 0 || k == 3) ? hl : -hl, z = (k < 2) ? hw : -hw;
    X = c * x + s * z + tx;
    Z = -s * x + c * z + tz;
}

// the area of (the polygon whose four corners the caller has stored in s_x[0][0..3][tid], s_z[0][0..3][tid]) clipped against the
// four edges of the rectangle (gX, gZ)
template <int THREADS>
__device__ __forceinline__ double intersection(double (*s_x)[kMaxVerts][THREADS], double (*s_z)[kMaxVerts][THREADS], int tid,
                                               const double (&gX)[4], const double (&gZ)[4])
{
    int n = 4, cur = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double ax = gX[e], az = gZ[e];
        const double ex = gX[(e + 1) & 3] - ax, ez = gZ[(e + 1) & 3] - az;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            const double px = s_x[cur][i][tid], pz = s_z[cur][i][tid];
            const double qx = s_x[cur][j][tid], qz = s_z[cur][j][tid];
            const double dp = ex * (pz - az) - ez * (px - ax);
            const double dq = ex * (qz - az) - ez * (qx - ax);
            const bool in_p = dp >= 0.0, in_q = dq >= 0.0;
            if (in_p && m < kMaxVerts) {
                s_x[cur ^ 1][m][tid] = px; s_z[cur ^ 1][m][tid] = pz;
                ++m;
            }
            if (in_p != in_q && m < kMaxVerts) {     // (a convex polygon gains one vertex per edge; the bound only guards the store)
                const double den = dq - dp;
                s_x[cur ^ 1][m][tid] = (px * dq - qx * dp) / den;
                s_z[cur ^ 1][m][tid] = (pz * dq - qz * dp) / den;
                ++m;
            }
        }
        n = m;
        cur ^= 1;
    }
    double twice = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        twice = twice + (s_x[cur][i][tid] * s_z[cur][j][tid] - s_x[cur][j][tid] * s_z[cur][i][tid]);
    }
    return n < 3 ? 0.0 : fabs(twice) / 2.0;
}

// the height term of the 3-D overlap: the two boxes stand on y (the bottom face, Y down) and reach up to y - h
__device__ __forceinline__ double height_overlap(double y_a, double h_a, double y_b, double h_b)
{
    const double top = (y_a - h_a) > (y_b - h_b) ? (y_a - h_a) : (y_b - h_b);
    const double hh = (y_a < y_b ? y_a : y_b) - top;
    return hh > 0.0 ? hh : 0.0;
}

}  // namespace rot_iou
