// The per-(detection, plane) arithmetic of ground-plane polling, shared by csrc/poll.hip (gpp_poll_f32: the selection) and
// csrc/plane_db.hip (gpp_poll_costs_u16: the cost table of the plane distillation): back-projection, poll targets, plane
// canonicalisation and the hypothesis of one pair.  float32, every operation separate (both files are compiled with -ffp-contract=off
// and without packed-FP32 instructions), evaluation order identical to oracle/polling_np.py / oracle/polling.c.
//
// Everything here is force-inlined into the including kernel: the header adds no kernel and no symbol of its own.
#pragma once

#include <hip/hip_runtime.h>

namespace {

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 scale3(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float norm3(V3 a) { return sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z); }
__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }

struct Hyp { V3 X[4]; float zc, votes, res; };

// fit_road_planes.py:84-109 for one (detection, plane) pair
__device__ __forceinline__ Hyp evaluate(const V3 (&ray)[4], float4 pl, const float (&target)[6], float thr)
{
    Hyp h;
    V3 n = {pl.x, pl.y, pl.z};
    float nd = -pl.w;
#pragma unroll
    for (int k = 0; k < 3; ++k) h.X[k] = scale3(ray[k], fabsf(nd / dot3(n, ray[k])));
    h.zc = cross3(sub3(h.X[0], h.X[1]), sub3(h.X[2], h.X[1])).y;
    V3 perp = cross3(ray[3], cross3(n, ray[3]));
    float num = dot3(perp, h.X[1]);
    float den = dot3(perp, n);
    h.X[3] = sub3(h.X[1], scale3(n, num / den));
    constexpr int seg[6][2] = {{1, 3}, {0, 1}, {1, 2}, {0, 2}, {0, 3}, {2, 3}};
    h.votes = 0.0f;
    h.res = 0.0f;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        float r = fabsf(norm3(sub3(h.X[seg[p][0]], h.X[seg[p][1]])) - target[p]);
        float v = (r > thr) ? 0.0f : 1.0f;
        h.votes = (p == 0) ? v : h.votes + v;
        h.res = (p == 0) ? r : h.res + r;
    }
    return h;
}

// fit_road_planes.py:75-77: normal up, unit norm
__device__ __forceinline__ float4 canonical_plane(float4 p)
{
    float dir = -sgn(p.y);
    float a = p.x * dir, b = p.y * dir, c = p.z * dir, d = p.w * dir;
    float nn = sqrtf((a * a + b * b) + c * c);
    return make_float4(a / nn, b / nn, c / nn, d / nn);
}

// fit_road_planes.py:80-83 back-projection of the four keypoints of one row: bx its 12 box values, Pi its image's P_inv (4, 3)
__device__ __forceinline__ void poll_rays(const float* bx, const float* Pi, V3 (&ray)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float x = bx[4 + 2 * k], y = bx[5 + 2 * k];
        float r0 = (Pi[0] * x + Pi[1] * y) + Pi[2] * 1.0f;
        float r1 = (Pi[3] * x + Pi[4] * y) + Pi[5] * 1.0f;
        float r2 = (Pi[6] * x + Pi[7] * y) + Pi[8] * 1.0f;
        float s = sgn(r2);
        ray[k] = {r0 * s, r1 * s, r2 * s};
    }
}

// fit_road_planes.py:61-73, 95-109 poll targets of one row (one_hot(-1) = 0 -> orientation dependent targets are 0)
__device__ __forceinline__ void poll_targets(const float* dm, int o, float (&target)[6])
{
    float h = dm[0], w = dm[1], l = dm[2];
    float hw = sqrtf(h * h + w * w), wl = sqrtf(w * w + l * l), hl = sqrtf(h * h + l * l);
    float oh0 = (o == 0) ? 1.0f : 0.0f, oh1 = (o == 1) ? 1.0f : 0.0f;
    float oh2 = (o == 2) ? 1.0f : 0.0f, oh3 = (o == 3) ? 1.0f : 0.0f;
#define GPP_MIX(a, b, c, d) (((oh0 * (a) + oh1 * (b)) + oh2 * (c)) + oh3 * (d))
    target[0] = h;
    target[1] = GPP_MIX(l, w, w, l);
    target[2] = GPP_MIX(w, l, l, w);
    target[3] = wl;
    target[4] = GPP_MIX(hl, hw, hw, hl);
    target[5] = GPP_MIX(hw, hl, hl, hw);
#undef GPP_MIX
}

}  // namespace
