// The two pooling layers of the Keras DenseNet backbone (keras.applications.densenet.DenseNet, instantiated at
// /root/reference/keras_retinanet_3D/models/densenet.py:62-94), float32 NHWC, each writing into a channel slice of a wider map
// (out_pitch >= C channels per output pixel): the first C channels of the next dense block's concatenation buffer.
//   ZeroPadding2D(1) + MaxPooling2D(3, strides=2) 'pool1'          gpp_maxpool3x3s2_pad_f32 (pad = 1: symmetric, explicit; the input is
//                                                                   post-ReLU, so zero and -inf padding give the same maximum)
//   AveragePooling2D(2, strides=2) 'poolS_pool' (valid: floor)      gpp_avgpool2x2_f32: the window summed in row-major order, then * 0.25
// The ResNet pool ('same' padding, gpp_maxpool3x3s2_same in stem.hip) is a different layer and keeps its kernel.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpp.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool AVG>
__global__ __launch_bounds__(256) void dense_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H, int W, int C,
                                                         int Ho, int Wo, int pad, int out_pitch)
{
    const int cv = C / 4;
    const int64_t total = (int64_t)B * Ho * Wo * cv;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(e % cv);
        int64_t p = e / cv;
        const int ox = (int)(p % Wo);
        p /= Wo;
        const int oy = (int)(p % Ho);
        const int b = (int)(p / Ho);
        const float* src = in + (int64_t)b * H * W * C + c4 * 4;
        f32x4 r;
        if constexpr (AVG) {
            // valid 2 x 2 window: Ho = H / 2, so rows 2 oy + 1 < H and columns 2 ox + 1 < W
            const float* p00 = src + ((int64_t)(2 * oy) * W + 2 * ox) * C;
            const f32x4 a = *(const f32x4*)p00, bb = *(const f32x4*)(p00 + C);
            const f32x4 c = *(const f32x4*)(p00 + (int64_t)W * C), d = *(const f32x4*)(p00 + (int64_t)W * C + C);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = (((a[k] + bb[k]) + c[k]) + d[k]) * 0.25f;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = -INFINITY;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int iy = oy * 2 - pad + dy;
                if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int ix = ox * 2 - pad + dx;
                    if ((unsigned)ix >= (unsigned)W) continue;
                    const f32x4 v = *(const f32x4*)(src + ((int64_t)iy * W + ix) * C);
#pragma unroll
                    for (int k = 0; k < 4; ++k) r[k] = fmaxf(r[k], v[k]);
                }
            }
        }
        *(f32x4*)(out + ((int64_t)b * Ho * Wo + (int64_t)oy * Wo + ox) * out_pitch + c4 * 4) = r;
    }
}

int check_args(const float* in, const float* out, int B, int H, int W, int C, int out_pitch)
{
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || out_pitch < C || out_pitch % 4 != 0) return GPP_ERR_BAD_ARG;
    if ((int64_t)B * H * W * C >= (1LL << 40)) return GPP_ERR_UNSUPPORTED;
    if (((uintptr_t)in | (uintptr_t)out) & 15) return GPP_ERR_ALIGN;
    return GPP_OK;
}

template <bool AVG>
int launch(const float* in, float* out, int B, int H, int W, int C, int Ho, int Wo, int pad, int out_pitch, void* stream)
{
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    dense_pool_kernel<AVG><<<blocks, 256, 0, (hipStream_t)stream>>>(in, out, B, H, W, C, Ho, Wo, pad, out_pitch);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int gpp_maxpool3x3s2_pad_f32(const float* in, float* out, int B, int H, int W, int C, int pad, int out_pitch, void* stream)
{
    int rc = check_args(in, out, B, H, W, C, out_pitch);
    if (rc != GPP_OK) return rc;
    if (pad < 0 || pad > 1) return GPP_ERR_UNSUPPORTED;          // (pad 2 would let a window see padding only)
    if (H + 2 * pad < 3 || W + 2 * pad < 3) return GPP_ERR_BAD_ARG;
    const int Ho = (H + 2 * pad - 3) / 2 + 1, Wo = (W + 2 * pad - 3) / 2 + 1;
    return launch<false>(in, out, B, H, W, C, Ho, Wo, pad, out_pitch, stream);
}

extern "C" int gpp_avgpool2x2_f32(const float* in, float* out, int B, int H, int W, int C, int out_pitch, void* stream)
{
    int rc = check_args(in, out, B, H, W, C, out_pitch);
    if (rc != GPP_OK) return rc;
    if (H < 2 || W < 2) return GPP_ERR_BAD_ARG;
    return launch<true>(in, out, B, H, W, C, H / 2, W / 2, 0, out_pitch, stream);
}
