// KITTI keypoint ("mod") labels from label_2 rows and the camera matrix on gfx950 (MI355X): one thread per (image, label row).
//
// Restates the reference's MATLAB label preparation:
//   label_prep/create_mod_labels.m   the 20 fields of a line, the demotion of an object behind the camera, the orientation class from
//                                    alpha and the keypoint <-> corner table :57-100
//   label_prep/computeBox3D.m        the eight corners :22-30, the Z < 0.1 rule :33
//   label_prep/projectToImage.m      P [X Y Z 1]^T and the two divisions :15-18
// (utils/label_prep.py is the host form; DESIGN.md section 4.18 is the specification.)  Layouts: include/gpp.h, gpp_label_prep_f64.
//
// Arithmetic: float64 throughout, every operation separate (this file is compiled with -ffp-contract=off).  cos(r_y) and sin(r_y) are
// INPUTS, computed once on the host for the host form and the device form alike: device libm, glibc and MATLAB each round the last
// bit of a cosine their own way, and with the two values given the kernel is left with + - * /, minimum, maximum and compares, all
// correctly rounded -- its result equals the NumPy form bit for bit.  Parity with MATLAB itself is UNPINNED (its cos / sin may differ
// in the last bit, which moves a pixel coordinate by about 1e-13).
//
// The eight corners live in named registers (four (X, Z) pairs, two heights); the four keypoint corners are selected by compares
// unrolled over the orientation class: no array indexed at run time, no scratch.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpp.h"

namespace {

constexpr int kThreads = 256;
constexpr double kDegPerRad = 180.0 / 3.141592653589793238462643383279502884;        // MATLAB's rad2deg: (180 / pi) * alpha

// one of four by the orientation class (create_mod_labels.m:57-100)
__host__ __device__ inline double pick(int o, double a0, double a1, double a2, double a3)
{
    return o == 0 ? a0 : (o == 1 ? a1 : (o == 2 ? a2 : a3));
}

__host__ __device__ inline double lower(double a, double b) { return b < a ? b : a; }
__host__ __device__ inline double upper(double a, double b) { return b > a ? b : a; }

struct Px { double x, y; };

// projectToImage.m: row-times-column sums in matmul order, then the two divisions
__host__ __device__ inline Px project(const double* __restrict__ P, double X, double Y, double Z)
{
    const double u = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
    const double v = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
    const double w = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
    return {u / w, v / w};
}

__global__ __launch_bounds__(kThreads) void label_prep_kernel(const double* __restrict__ labels, const int32_t* __restrict__ label_counts,
                                                              const double* __restrict__ Pm, const double* __restrict__ trig, int64_t total, int A,
                                                              uint32_t det_types, int own_box, double* __restrict__ mod,
                                                              float* __restrict__ boxes, float* __restrict__ dims, float* __restrict__ scores,
                                                              int32_t* __restrict__ det_labels, int32_t* __restrict__ orient)
{
    const int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (row >= total) return;
    const int64_t b = row / A;
    const int a = (int)(row - b * A);
    double* __restrict__ out = mod + row * GPP_LABEL_MOD_COLS;
    int count = label_counts[b];
    count = count < 0 ? 0 : (count > A ? A : count);

    bool detection = false;
    int o = -1;
    double x1 = -1.0, y1 = -1.0, x2 = -1.0, y2 = -1.0, own_x1 = -1.0, own_y1 = -1.0, own_x2 = -1.0, own_y2 = -1.0;
    double xl = -1.0, yl = -1.0, xm = -1.0, ym = -1.0, xr = -1.0, yr = -1.0, xt = -1.0, yt = -1.0, h = -1.0, w = -1.0, l = -1.0;
    if (a >= count) {
#pragma unroll
        for (int k = 0; k < GPP_LABEL_MOD_COLS; ++k) out[k] = -1.0;
    } else {
        const double* __restrict__ g = labels + row * GPP_KITTI_LABEL_COLS;
        const double* __restrict__ P = Pm + b * 12;
        const double kind = g[0], alpha = g[3];
        own_x1 = g[4]; own_y1 = g[5]; own_x2 = g[6]; own_y2 = g[7];
        h = g[8]; w = g[9]; l = g[10];
        const double tx = g[11], ty = g[12], tz = g[13];
        const double c = trig[row * 2], s = trig[row * 2 + 1];
        // computeBox3D.m:22-30.  Corners 1-4 (bottom): (x, z) = (l/2, w/2) (l/2, -w/2) (-l/2, -w/2) (-l/2, w/2); corners 5-8 the same at y = -h
        const double hl = l / 2.0, hw = w / 2.0, ns = -s;
        const double X1 = (c * hl + s * hw) + tx, Z1 = (ns * hl + c * hw) + tz;
        const double X2 = (c * hl + s * (-hw)) + tx, Z2 = (ns * hl + c * (-hw)) + tz;
        const double X3 = (c * (-hl) + s * (-hw)) + tx, Z3 = (ns * (-hl) + c * (-hw)) + tz;
        const double X4 = (c * (-hl) + s * hw) + tx, Z4 = (ns * (-hl) + c * hw) + tz;
        const double Yb = 0.0 + ty, Yt = (-h) + ty;
        const bool behind = (Z1 < 0.1) || (Z2 < 0.1) || (Z3 < 0.1) || (Z4 < 0.1);                  // :33
        const double deg = kDegPerRad * alpha;
        if (deg >= 0.0 && deg < 90.0) o = 0;
        else if (deg >= 90.0 && deg < 180.0) o = 1;
        else if (deg >= -90.0 && deg < 0.0) o = 2;
        else if (deg >= -180.0 && deg < -90.0) o = 3;
        if (behind || o < 0) {
            // create_mod_labels.m:37-55 (an alpha outside [-180, 180) degrees is out of contract: the script would reuse the previous
            // object's variables; the row is demoted here, the host reader raises)
            o = -1;
            out[0] = 2.0; out[1] = -1.0; out[2] = -1.0; out[3] = -10.0;
            out[4] = own_x1; out[5] = own_y1; out[6] = own_x2; out[7] = own_y2;
#pragma unroll
            for (int k = 8; k < 16; ++k) out[k] = -10000.0;
            out[16] = h; out[17] = w; out[18] = l; out[19] = -1.0;
        } else {
            const Px p1 = project(P, X1, Yb, Z1), p2 = project(P, X2, Yb, Z2), p3 = project(P, X3, Yb, Z3), p4 = project(P, X4, Yb, Z4);
            const Px p5 = project(P, X1, Yt, Z1), p6 = project(P, X2, Yt, Z2), p7 = project(P, X3, Yt, Z3), p8 = project(P, X4, Yt, Z4);
            // :57-100: l m r t = corners 3 2 1 6 | 2 1 4 5 | 4 3 2 7 | 1 4 3 8
            xl = pick(o, p3.x, p2.x, p4.x, p1.x); yl = pick(o, p3.y, p2.y, p4.y, p1.y);
            xm = pick(o, p2.x, p1.x, p3.x, p4.x); ym = pick(o, p2.y, p1.y, p3.y, p4.y);
            xr = pick(o, p1.x, p4.x, p2.x, p3.x); yr = pick(o, p1.y, p4.y, p2.y, p3.y);
            xt = pick(o, p6.x, p5.x, p7.x, p8.x); yt = pick(o, p6.y, p5.y, p7.y, p8.y);
            // :102-105, unclipped
            x1 = lower(lower(lower(lower(lower(lower(lower(p1.x, p2.x), p3.x), p4.x), p5.x), p6.x), p7.x), p8.x);
            y1 = lower(lower(lower(lower(lower(lower(lower(p1.y, p2.y), p3.y), p4.y), p5.y), p6.y), p7.y), p8.y);
            x2 = upper(upper(upper(upper(upper(upper(upper(p1.x, p2.x), p3.x), p4.x), p5.x), p6.x), p7.x), p8.x);
            y2 = upper(upper(upper(upper(upper(upper(upper(p1.y, p2.y), p3.y), p4.y), p5.y), p6.y), p7.y), p8.y);
            out[0] = kind; out[1] = g[1]; out[2] = g[2]; out[3] = alpha;
            out[4] = x1; out[5] = y1; out[6] = x2; out[7] = y2;
            out[8] = xl; out[9] = yl; out[10] = xm; out[11] = ym; out[12] = xr; out[13] = yr; out[14] = xt; out[15] = yt;
            out[16] = h; out[17] = w; out[18] = l; out[19] = (double)o;
            detection = kind >= 0.0 && kind < 32.0 && ((det_types >> (uint32_t)kind) & 1u) != 0u;
        }
    }
    if (!boxes) return;
    float* __restrict__ bx = boxes + row * 12;
    float* __restrict__ dm = dims + row * 3;
    if (detection) {
        bx[0] = (float)(own_box ? own_x1 : x1); bx[1] = (float)(own_box ? own_y1 : y1);
        bx[2] = (float)(own_box ? own_x2 : x2); bx[3] = (float)(own_box ? own_y2 : y2);
        bx[4] = (float)xl; bx[5] = (float)yl; bx[6] = (float)xm; bx[7] = (float)ym;
        bx[8] = (float)xr; bx[9] = (float)yr; bx[10] = (float)xt; bx[11] = (float)yt;
        dm[0] = (float)h; dm[1] = (float)w; dm[2] = (float)l;
        scores[row] = 1.0f; det_labels[row] = 0; orient[row] = o;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) bx[k] = -1.0f;
        dm[0] = -1.0f; dm[1] = -1.0f; dm[2] = -1.0f;
        scores[row] = -1.0f; det_labels[row] = -1; orient[row] = -1;
    }
}

}  // namespace

extern "C" int gpp_label_prep_f64(const double* labels, const int32_t* label_counts, const double* P, const double* trig, int B, int A,
                                  unsigned det_types, int own_box, double* mod,
                                  float* boxes, float* dims, float* scores, int32_t* det_labels, int32_t* orientations, void* stream)
{
    if (B < 0 || A < 0) return GPP_ERR_BAD_ARG;
    const int given = (boxes != nullptr) + (dims != nullptr) + (scores != nullptr) + (det_labels != nullptr) + (orientations != nullptr);
    if (given != 0 && given != 5) return GPP_ERR_BAD_ARG;
    if (B == 0 || A == 0) return GPP_OK;
    if (!labels || !label_counts || !P || !trig || !mod) return GPP_ERR_BAD_ARG;
    const int64_t total = (int64_t)B * A;
    const int64_t blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return GPP_ERR_UNSUPPORTED;
    label_prep_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(labels, label_counts, P, trig, total, A, (uint32_t)det_types,
                                                                                         own_box, mod, boxes, dims, scores, det_labels, orientations);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
