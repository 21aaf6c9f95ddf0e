// The ragged form of preprocess.hip (gpp_preprocess_u8_bgr_ragged): uint8 BGR frames of different raw sizes that resize into one height
// class -> the float32 canvas the ragged stem reads (stem.hip).  A translation unit of its own, compiled like
// preprocess.hip (-ffp-contract=off), so that preprocess_kernel stays exactly the code it was.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpp.h"

namespace {

// Ragged batches: frame b is stored densely (its own h_b x w_b x 3 bytes) at the start of slot b of a uint8 canvas of
// H x W x 3 bytes per slot; raw_hw[b] = (h_b, w_b); the taps are per image ([B][Ho] and [B][Wo]); heights[b] = the image's resized
// height: rows below it are written as zero (the padding the ragged stem never reads as data).  The arithmetic is preprocess_kernel's.
// Sizes and taps are device data: they are clamped, so that whatever they hold no access leaves the slot.
__global__ __launch_bounds__(256) void preprocess_ragged_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                                const int32_t* __restrict__ raw_hw, const int32_t* __restrict__ heights,
                                                                const int32_t* __restrict__ y0, const int32_t* __restrict__ y1,
                                                                const float* __restrict__ wy, const int32_t* __restrict__ x0,
                                                                const int32_t* __restrict__ x1, const float* __restrict__ wx,
                                                                int H, int W, int Ho, int Wo, float m0, float m1, float m2)
{
    const int b = blockIdx.z, oy = blockIdx.y;
    const int ox = blockIdx.x * 256 + threadIdx.x;
    if (ox >= Wo) return;
    float* dst = out + (((size_t)b * Ho + oy) * Wo + ox) * 3;
    const int hb = min(max(heights[b], 1), Ho);
    if (oy >= hb) {
        dst[0] = 0.0f;
        dst[1] = 0.0f;
        dst[2] = 0.0f;
        return;
    }
    const int h = min(max(raw_hw[2 * b], 1), H), w = min(max(raw_hw[2 * b + 1], 1), W);
    const uint8_t* img = in + (size_t)b * H * W * 3;
    const size_t to = (size_t)b * Ho + oy, tx = (size_t)b * Wo + ox;
    const uint8_t* r0 = img + (size_t)min(max(y0[to], 0), h - 1) * w * 3;
    const uint8_t* r1 = img + (size_t)min(max(y1[to], 0), h - 1) * w * 3;
    const int xa = min(max(x0[tx], 0), w - 1) * 3, xb = min(max(x1[tx], 0), w - 1) * 3;
    const float fx = wx[tx], fy = wy[to];
    const float mean[3] = {m0, m1, m2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (float)r0[xa + c] - mean[c], bb = (float)r0[xb + c] - mean[c];
        const float cc = (float)r1[xa + c] - mean[c], dd = (float)r1[xb + c] - mean[c];
        const float top = a * (1.0f - fx) + bb * fx;
        const float bot = cc * (1.0f - fx) + dd * fx;
        dst[c] = top * (1.0f - fy) + bot * fy;
    }
}

}  // namespace

extern "C" int gpp_preprocess_u8_bgr_ragged(const uint8_t* frames, float* out, const int32_t* raw_hw, const int32_t* heights,
                                            const int32_t* y0, const int32_t* y1, const float* wy,
                                            const int32_t* x0, const int32_t* x1, const float* wx, int B, int H, int W, int Hp, int Ho, int Wo,
                                            float mean_b, float mean_g, float mean_r, void* stream)
{
    if (!frames || !out || !raw_hw || !heights || !y0 || !y1 || !wy || !x0 || !x1 || !wx) return GPP_ERR_BAD_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || Ho > 65535 || B > 65535) return GPP_ERR_BAD_ARG;
    if (Hp <= 0 || Ho != 4 * Hp) return GPP_ERR_BAD_ARG;                     // the canvas rows are those of the height class
    if (((uintptr_t)out | (uintptr_t)raw_hw | (uintptr_t)heights | (uintptr_t)y0 | (uintptr_t)y1 | (uintptr_t)wy | (uintptr_t)x0 |
         (uintptr_t)x1 | (uintptr_t)wx) & 3) return GPP_ERR_ALIGN;
    preprocess_ragged_kernel<<<dim3((unsigned)((Wo + 255) / 256), (unsigned)Ho, (unsigned)B), 256, 0, (hipStream_t)stream>>>(
        frames, out, raw_hw, heights, y0, y1, wy, x0, x1, wx, H, W, Ho, Wo, mean_b, mean_g, mean_r);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
