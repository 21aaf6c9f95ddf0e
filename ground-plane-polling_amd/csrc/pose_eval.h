// The location that pose recovery gives one (object, plane) hypothesis, and its error against a label, for csrc/plane_db.hip
// (gpp_pose_costs_u16): the live branch of utils/gpp_utils.recover_pose written out by components on the four
// keypoints of poll_eval.h's evaluate().  float32, every operation separate (the including file is compiled with -ffp-contract=off and
// without packed-FP32 instructions), evaluation order identical to utils/plane_db.pair_costs_np.
//
// Everything here is force-inlined into the including kernel: the header adds no kernel and no symbol of its own.
#pragma once

#include <hip/hip_runtime.h>

#include "poll_eval.h"

namespace {

__device__ __forceinline__ V3 add3(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 div3(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }

// the bottom-face centre of the cuboid that the keypoints X_l, X_m, X_r, X_t span: o the orientation class 0..3, w the width
__device__ __forceinline__ V3 pose_location(const V3 (&X)[4], int o, float w)
{
    const V3 X_m = X[1], X_t = X[3];
    const V3 X_s = (o == 0 || o == 3) ? X[0] : X[2];             // the second bottom keypoint that is used
    const float h = norm3(sub3(X_t, X_m));
    const float e = norm3(sub3(X_s, X_m));
    const V3 y = div3(sub3(X_m, X_t), h);
    const float sx = (o == 0 || o == 1) ? 1.0f : -1.0f;
    const V3 x = div3(scale3(sub3(X_m, X_s), sx), e);
    const V3 z = cross3(x, y);
    const float sz = (o == 0 || o == 2) ? 1.0f : -1.0f;
    return add3(div3(add3(X_m, X_s), 2.0f), div3(scale3(scale3(z, sz), w), 2.0f));
}

// the error in quanta of 1/256 m, saturating at 65534 (a NaN or infinite distance fails the comparison: 65534 too)
__device__ __forceinline__ unsigned pose_error_quanta(const V3 (&X)[4], int o, float w, V3 want)
{
    const float dist = norm3(sub3(pose_location(X, o, w), want));
    const float s = dist * 256.0f;
    return (s < 65534.0f) ? (unsigned)(int)s : 65534u;
}

}  // namespace
