// The ground-plane Kalman filter of DESIGN.md section 4.34 as __device__ functions: the only place where its expressions are device code.
// csrc/track.hip (the tracker, one thread per slot, the mean in LDS) and csrc/track_smooth.hip (the offline smoother's forward pass, one
// lane per segment, the mean in registers) call them on their own storage; csrc/pose.hip takes wrap.  utils/track_kf.py is the NumPy
// form, tests/track_kf_oracle.py and tests/track_smooth_oracle.py the loop-written oracles.  Every + - * / and sqrt is one separately
// rounded float64 operation in the association written here: the units that include this are compiled with -ffp-contract=off, and the
// tests compare words with ==.  The host half: what both entry points refuse of a gpp_track_kf_params and of one ego record.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#include "gpp.h"

namespace gpp_kf {

constexpr double kPi = 3.141592653589793238462643383279502884;
constexpr double kTwoPi = 2.0 * kPi;

enum { AXX = 0, AXZ, AZZ, BXX, BXZ, BZX, BZZ, CXX, CXZ, CZZ };       // gpp_track_cov's fields
constexpr int kCov = GPP_TRACK_COV_FIELDS;
static_assert(CZZ + 1 == kCov, "the ten words of section 4.34");

// run_network.py:312-316: a % 2 pi (Python: the sign of the divisor), then into [-pi, pi)
__host__ __device__ __forceinline__ double wrap(double a)
{
    a = a - kTwoPi * floor(a / kTwoPi);
    if (a < 0.0) a += kTwoPi;
    if (a >= kTwoPi) a -= kTwoPi;
    if (a >= kPi) a -= kTwoPi;
    return a;
}

// "row noise": sigma radial0 + radial1 rho along the row's viewing ray on the ground plane, tangential0 + tangential1 rho across it
__device__ __forceinline__ void row_noise(double x, double z, const gpp_track_kf_params& kf, double& rxx, double& rxz, double& rzz)
{
    const double rho = sqrt((x * x) + (z * z));
    double ux = 0.0, uz = 1.0;
    if (rho != 0.0) { ux = x / rho; uz = z / rho; }
    const double sr = kf.radial0 + (kf.radial1 * rho), st = kf.tangential0 + (kf.tangential1 * rho);
    const double vr = sr * sr, vt = st * st;
    const double dv = vr - vt;
    rxx = vt + (dv * (ux * ux));
    rxz = dv * (ux * uz);
    rzz = vt + (dv * (uz * uz));
}

// "births": A = R of the row, B = 0, C = birth_speed^2 I
__device__ __forceinline__ void born_cov(double (&P)[kCov], double rxx, double rxz, double rzz, double speed)
{
    P[AXX] = rxx; P[AXZ] = rxz; P[AZZ] = rzz;
    P[BXX] = 0.0; P[BXZ] = 0.0; P[BZX] = 0.0; P[BZZ] = 0.0;
    P[CXX] = speed * speed; P[CXZ] = 0.0; P[CZZ] = speed * speed;
}

// "1 predict": P = F P F^T + Q, all from the old values
__device__ __forceinline__ void predict_cov(double (&P)[kCov], double q_pos, double q_vel)
{
    const double axx = ((P[AXX] + (P[BXX] + P[BXX])) + P[CXX]) + q_pos;
    const double axz = (P[AXZ] + (P[BXZ] + P[BZX])) + P[CXZ];
    const double azz = ((P[AZZ] + (P[BZZ] + P[BZZ])) + P[CZZ]) + q_pos;
    const double bxx = P[BXX] + P[CXX], bxz = P[BXZ] + P[CXZ], bzx = P[BZX] + P[CXZ], bzz = P[BZZ] + P[CZZ];
    P[AXX] = axx; P[AXZ] = axz; P[AZZ] = azz;
    P[BXX] = bxx; P[BXZ] = bxz; P[BZX] = bzx; P[BZZ] = bzz;
    P[CXX] = P[CXX] + q_vel; P[CZZ] = P[CZZ] + q_vel;
}

// "ego": X -> Rg X Rg^T for a general 2 x 2 block (xx xz zx zz), every product and sum separate: (Rg X) first, then (Rg X) Rg^T
__device__ __forceinline__ void turn(double g00, double g01, double g10, double g11, double xx, double xz, double zx, double zz,
                                     double& oxx, double& oxz, double& ozx, double& ozz)
{
    const double mxx = (g00 * xx) + (g01 * zx), mxz = (g00 * xz) + (g01 * zz);
    const double mzx = (g10 * xx) + (g11 * zx), mzz = (g10 * xz) + (g11 * zz);
    oxx = (mxx * g00) + (mxz * g01);
    oxz = (mxx * g10) + (mxz * g11);
    ozx = (mzx * g00) + (mzz * g01);
    ozz = (mzx * g10) + (mzz * g11);
}

// "1b": the ground part of the ego record's rotation on the blocks A, B and C
__device__ __forceinline__ void turn_cov(double (&P)[kCov], double g00, double g01, double g10, double g11)
{
    double unused;                                       // (the lower triangle of a symmetric block is not kept)
    turn(g00, g01, g10, g11, P[AXX], P[AXZ], P[AXZ], P[AZZ], P[AXX], P[AXZ], unused, P[AZZ]);
    turn(g00, g01, g10, g11, P[BXX], P[BXZ], P[BZX], P[BZZ], P[BXX], P[BXZ], P[BZX], P[BZZ]);
    turn(g00, g01, g10, g11, P[CXX], P[CXZ], P[CXZ], P[CZZ], P[CXX], P[CXZ], unused, P[CZZ]);
}

// "5 update" of the predicted mean (x, z, vx, vz) and P with a row of noise R that lies (dx, dz) from the predicted position.  False,
// and nothing changed, when det S is not > 0: the caller takes its own fallback
__device__ __forceinline__ bool update(double (&P)[kCov], double rxx, double rxz, double rzz, double dx, double dz,
                                       double& x, double& z, double& vx, double& vz)
{
    const double sxx = P[AXX] + rxx, sxz = P[AXZ] + rxz, szz = P[AZZ] + rzz;
    const double det = (sxx * szz) - (sxz * sxz);
    if (!(det > 0.0)) return false;
    const double ixx = szz / det, ixz = -(sxz / det), izz = sxx / det;
    const double kxx = (P[AXX] * ixx) + (P[AXZ] * ixz), kxz = (P[AXX] * ixz) + (P[AXZ] * izz);
    const double kzx = (P[AXZ] * ixx) + (P[AZZ] * ixz), kzz = (P[AXZ] * ixz) + (P[AZZ] * izz);
    const double lxx = (P[BXX] * ixx) + (P[BZX] * ixz), lxz = (P[BXX] * ixz) + (P[BZX] * izz);
    const double lzx = (P[BXZ] * ixx) + (P[BZZ] * ixz), lzz = (P[BXZ] * ixz) + (P[BZZ] * izz);
    x = x + ((kxx * dx) + (kxz * dz));
    z = z + ((kzx * dx) + (kzz * dz));
    vx = vx + ((lxx * dx) + (lxz * dz));
    vz = vz + ((lzx * dx) + (lzz * dz));
    const double axx = P[AXX] - ((kxx * P[AXX]) + (kxz * P[AXZ]));
    const double axz = P[AXZ] - ((kxx * P[AXZ]) + (kxz * P[AZZ]));
    const double azz = P[AZZ] - ((kzx * P[AXZ]) + (kzz * P[AZZ]));
    const double bxx = P[BXX] - ((kxx * P[BXX]) + (kxz * P[BZX]));
    const double bxz = P[BXZ] - ((kxx * P[BXZ]) + (kxz * P[BZZ]));
    const double bzx = P[BZX] - ((kzx * P[BXX]) + (kzz * P[BZX]));
    const double bzz = P[BZZ] - ((kzx * P[BXZ]) + (kzz * P[BZZ]));
    const double cxx = P[CXX] - ((lxx * P[BXX]) + (lxz * P[BZX]));
    const double cxz = P[CXZ] - ((lxx * P[BXZ]) + (lxz * P[BZZ]));
    const double czz = P[CZZ] - ((lzx * P[BXZ]) + (lzz * P[BZZ]));
    P[AXX] = axx; P[AXZ] = axz; P[AZZ] = azz;
    P[BXX] = bxx; P[BXZ] = bxz; P[BZX] = bzx; P[BZZ] = bzz;
    P[CXX] = cxx; P[CXZ] = cxz; P[CZZ] = czz;
    return true;
}

// ---- the host half: each entry point keeps its own loop bounds and its place in the check order

// what gpp_track_kf_f64 and gpp_track_smooth_f64 refuse of the filter's parameters (a NaN is neither positive nor not negative)
inline bool kf_params_bad(const gpp_track_kf_params& k)
{
    const auto positive = [](double v) { return v > 0.0 && __builtin_isfinite(v); };
    const auto not_negative = [](double v) { return v >= 0.0 && __builtin_isfinite(v); };
    return !positive(k.radial0) || !positive(k.tangential0) || !positive(k.birth_speed) || !not_negative(k.radial1) ||
           !not_negative(k.tangential1) || !not_negative(k.q_pos) || !not_negative(k.q_vel) || k.reserved != 0;
}

// what they refuse of one ego record: R row-major, t and dyaw must be finite, the three words behind them 0
inline bool ego_record_bad(const double* e)
{
    for (int k = 0; k < 13; ++k)
        if (!__builtin_isfinite(e[k])) return true;
    for (int k = 13; k < GPP_TRACK_EGO_FIELDS; ++k)
        if (!(e[k] == 0.0)) return true;                 // (a NaN is not zero either)
    return false;
}

}  // namespace gpp_kf
