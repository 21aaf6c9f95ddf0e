// ResNet stem on gfx950: 7x7 stride-2 convolution of the 3-channel float32 input image with the
// frozen BatchNormalization folded in, ReLU, 16-bit NHWC output; and the 3x3 stride-2 'same'
// max-pool that follows it.
//
// Replaces (third-party keras_resnet, instantiated at
// /root/reference/keras_retinanet_3D/models/resnet.py:88-93):
//   ZeroPadding2D(3) -> Conv2D(64, 7x7, stride 2, valid, no bias) 'conv1' -> BatchNormalization
//   (eps 1e-5, frozen) 'bn_conv1' -> ReLU -> MaxPooling2D(3x3, stride 2, 'same') 'pool1'
//
// K = 7*7*3 = 147 is too thin for the 64-channel implicit-GEMM path; this version keeps the
// contraction on the vector ALUs in float32: a workgroup owns a 4-row x 64-column tile of
// output pixels, stages the (13 x 133 x 3) input patch in LDS once, and every lane computes
// all 64 output channels of one pixel with the weights broadcast from scalar registers.

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>

#include <atomic>

#include "gpp.h"
#include "conv_igemm_types.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) float f32x8_natural;
typedef f32x8_natural f32x8 __attribute__((aligned(16)));     // 8 floats, accessed as two 16-byte halves (GPP_F32 maps)

constexpr int TW = 64, TH = 4;                 // output tile
constexpr int kMaxStemDim = 1 << 20;           // batch, height, width of a launch: far beyond any image, far below overflow of the tile counts
constexpr int PW = TW * 2 + 5, PH = TH * 2 + 5;  // input patch
constexpr int PPITCH = PW * 3 + 1;             // floats per patch row (odd: spreads LDS banks)

// ---- ragged batches ----------------------------------------------------------------
// Every kernel of stem_kernels.h has a second, RAGGED form under a kernel symbol of its own (X_ragged_kernel beside X_kernel; the header
// is included twice, and the uniform kernels keep their names and, instruction for instruction, their code): the images of a batch share the canvas (B, H, W, 3) with H = 4 Hp rows and differ in their own height, read from an
// int32 table in device memory (data, not a launch argument: one plan, one captured graph for every mix of heights).  Image b
// occupies rows [0, H_b) of slot b; rows >= H_b are never read as data, they are the zero padding below the image.  Ho_b and the
// pool's pad_top follow from H_b; the pooled map has the Hp rows of the class for every image.  The table is clamped into
// [1, H], so whatever it holds, no access leaves the canvas.
__device__ __forceinline__ int ragged_height(const int* __restrict__ heights, int b, int H)
{
    // b is the same for the whole wavefront: keep the height (and what follows from it) in scalar registers -- the fused x3 kernel has no
    // vector register to spare
    const int h = __builtin_amdgcn_readfirstlane(heights[b]);
    return h < 1 ? 1 : (h > H ? H : h);
}
// (where b differs from lane to lane: the max pool)
__device__ __forceinline__ int ragged_height_of_lane(const int* __restrict__ heights, int b, int H)
{
    const int h = heights[b];
    return h < 1 ? 1 : (h > H ? H : h);
}
__device__ __forceinline__ int pool_pad_top(int Hp, int Ho)
{
    const int need = (Hp - 1) * 2 + 3 - Ho;
    return (need > 0 ? need : 0) / 2;
}

// the kernels, in both forms (stem_kernels.h)
#define STEM_RAGGED 0
#define STEM_K(name) name##_kernel
#define STEM_HEIGHTS_ARG
#define STEM_FORM constexpr bool RAGGED = false; constexpr const int* heights = nullptr; (void)heights
#include "stem_kernels.h"
#undef STEM_RAGGED
#undef STEM_K
#undef STEM_HEIGHTS_ARG
#undef STEM_FORM
#define STEM_RAGGED 1
#define STEM_K(name) name##_ragged_kernel
#define STEM_HEIGHTS_ARG , const int* __restrict__ heights
#define STEM_FORM constexpr bool RAGGED = true
#include "stem_kernels.h"
#undef STEM_RAGGED
#undef STEM_K
#undef STEM_HEIGHTS_ARG
#undef STEM_FORM

template <typename scalar, typename vec8>
__global__ __launch_bounds__(256) void relu_kernel(const scalar* __restrict__ in, int64_t in_bs, scalar* __restrict__ out,
                                                   int64_t out_bs, int64_t n8)
{
    const scalar* src = in + (int64_t)blockIdx.y * in_bs;
    scalar* dst = out + (int64_t)blockIdx.y * out_bs;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n8; e += (int64_t)gridDim.x * 256) {
        vec8 v = *(const vec8*)(src + e * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = (scalar)fmaxf((float)v[c], 0.0f);
        *(vec8*)(dst + e * 8) = v;
    }
}

// ReLU on a pre-split GPP_BF16X3 map: every 128 bytes are [32 bf16 hi | 32 bf16 lo] of 32 channels, value = hi + lo with
// |lo| <= ulp(hi) / 2, so the sign of the value is the sign of hi: a negative hi clears the pair, everything else stays.
__global__ __launch_bounds__(256) void relu_x3_kernel(const char* __restrict__ in, int64_t in_bs_bytes, char* __restrict__ out,
                                                      int64_t out_bs_bytes, int64_t groups)
{
    const char* src = in + (int64_t)blockIdx.y * in_bs_bytes;
    char* dst = out + (int64_t)blockIdx.y * out_bs_bytes;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t off = (g >> 2) * 128 + (g & 3) * 16;       // 8 channels: 16 bytes of hi, their lo 64 bytes further
        bf16x8 h = *(const bf16x8*)(src + off), l = *(const bf16x8*)(src + off + 64);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool neg = (float)h[c] < 0.0f;
            h[c] = neg ? (__bf16)0.0f : h[c];
            l[c] = neg ? (__bf16)0.0f : l[c];
        }
        *(bf16x8*)(dst + off) = h;
        *(bf16x8*)(dst + off + 64) = l;
    }
}

inline int result()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

// what the host can see of a ragged call: the table pointer, and that the rows of the canvas (or of the conv map: rows_per_hp = 2) are
// those of the height class.  The heights themselves are device data (the kernels clamp them into the canvas).
inline int ragged_check(const int32_t* heights, int rows, int Hp, int rows_per_hp)
{
    if (!heights || Hp <= 0 || Hp > (1 << 24) || rows != rows_per_hp * Hp) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)heights & 3) return GPP_ERR_ALIGN;
    return GPP_OK;
}

// the entry points below in both forms: heights == nullptr is the uniform call (the kernels that existed before the ragged form)
int stem_f32_run(const float* in, const float* weight, const float* bias, void* out, int dtype, int B, int H, int W,
                 const int32_t* heights, void* stream)
{
    if (!in || !weight || !bias || !out || B <= 0 || H <= 0 || W <= 0) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)out) & 15) return GPP_ERR_ALIGN;
    if (B > kMaxStemDim || H > kMaxStemDim || W > kMaxStemDim) return GPP_ERR_UNSUPPORTED;      // (the tile arithmetic below stays inside an int)
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    if ((int64_t)((Wo + TW - 1) / TW) * ((Ho + TH - 1) / TH) >= (1LL << 30)) return GPP_ERR_UNSUPPORTED;
    dim3 grid((unsigned)(((Wo + TW - 1) / TW) * ((Ho + TH - 1) / TH)), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != GPP_BF16 && dtype != GPP_F16 && dtype != GPP_F32) return GPP_ERR_UNSUPPORTED;
    if (heights) {
        if (dtype == GPP_BF16)
            stem_ragged_kernel<__bf16, bf16x8><<<grid, 256, 0, st>>>(in, weight, bias, (__bf16*)out, H, W, Ho, Wo, heights);
        else if (dtype == GPP_F16)
            stem_ragged_kernel<_Float16, f16x8><<<grid, 256, 0, st>>>(in, weight, bias, (_Float16*)out, H, W, Ho, Wo, heights);
        else
            stem_ragged_kernel<float, f32x8><<<grid, 256, 0, st>>>(in, weight, bias, (float*)out, H, W, Ho, Wo, heights);
    } else if (dtype == GPP_BF16)
        stem_kernel<__bf16, bf16x8><<<grid, 256, 0, st>>>(in, weight, bias, (__bf16*)out, H, W, Ho, Wo);
    else if (dtype == GPP_F16)
        stem_kernel<_Float16, f16x8><<<grid, 256, 0, st>>>(in, weight, bias, (_Float16*)out, H, W, Ho, Wo);
    else
        stem_kernel<float, f32x8><<<grid, 256, 0, st>>>(in, weight, bias, (float*)out, H, W, Ho, Wo);
    return result();
}

}  // namespace

extern "C" int gpp_stem_conv7x7_bn_relu(const float* in, const float* weight, const float* bias, void* out, int dtype,
                                        int B, int H, int W, void* stream)
{
    return stem_f32_run(in, weight, bias, out, dtype, B, H, W, nullptr, stream);
}

extern "C" int gpp_stem_conv7x7_bn_relu_ragged(const float* in, const float* weight, const float* bias, void* out, int dtype,
                                               int B, int H, int W, int Hp, const int32_t* heights, void* stream)
{
    const int rc = ragged_check(heights, H, Hp, 4);
    return rc != GPP_OK ? rc : stem_f32_run(in, weight, bias, out, dtype, B, H, W, heights, stream);
}

#ifdef GPP_STAMPS
extern "C" int gpp_debug_set_stem_stamps(void* buffer)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stem_stamps), &buffer, sizeof(buffer));
}
#endif

extern "C" int gpp_stem_pack_weights_f16(const float* host_weight_147x64, void* host_packed, size_t packed_bytes)
{
    // host-side helper: [147][64] float32 (HWIO flattened, BN scale folded) -> [64][232] f16, rows interleaved as for
    // gpp_conv2d_igemm (row 16h + 4q + r of a 32-group = channel 8q + 4h + r), k = kh*32 + kw*3 + c, zero padded
    if (!host_weight_147x64 || !host_packed || packed_bytes < (size_t)64 * MW_PITCH * 2) return GPP_ERR_BAD_ARG;
    _Float16* dst = (_Float16*)host_packed;
    for (int pos = 0; pos < 64; ++pos) {
        const int g = pos / 32, within = pos % 32, h = within / 16, q = (within % 16) / 4, r = within % 4;
        const int n = g * 32 + 8 * q + 4 * h + r;
        for (int k = 0; k < MW_PITCH; ++k) {
            const int kh = k / 32, kc = k % 32;
            float v = 0.0f;
            if (k < 224 && kc < 21) v = host_weight_147x64[(kh * 21 + kc) * 64 + n];
            dst[pos * MW_PITCH + k] = (_Float16)v;
        }
    }
    return GPP_OK;
}

extern "C" int gpp_stem_pack_weights_f16x3(const float* host_weight_147x64, void* host_packed, size_t packed_bytes)
{
    // host-side helper: [147][64] float32 -> [whi 64 x 232 halfs][wlo 64 x 232 halfs][64 float32 out_scale]; channel n's weights are
    // multiplied by 2^k(n) (largest weight of the channel in [2^13, 2^14)) before they are split into two halves, out_scale[n] =
    // 2^-k(n); rows interleaved and k ordered as gpp_stem_pack_weights_f16
    const size_t need = (size_t)2 * 64 * MW_PITCH * 2 + 64 * sizeof(float);
    if (!host_weight_147x64 || !host_packed || packed_bytes < need) return GPP_ERR_BAD_ARG;
    _Float16* hi = (_Float16*)host_packed;
    _Float16* lo = hi + 64 * MW_PITCH;
    float* out_scale = (float*)(lo + 64 * MW_PITCH);
    for (int pos = 0; pos < 64; ++pos) {
        const int g = pos / 32, within = pos % 32, h = within / 16, q = (within % 16) / 4, r = within % 4;
        const int n = g * 32 + 8 * q + 4 * h + r;
        float amax = 0.0f;
        for (int k = 0; k < 147; ++k) amax = fmaxf(amax, fabsf(host_weight_147x64[k * 64 + n]));
        int e = 0;
        if (amax > 0.0f) { (void)frexpf(amax, &e); e = 14 - e; }          // amax = m * 2^(14 - e_new), m in [0.5, 1) -> amax * 2^e in [2^13, 2^14)
        // bounded as layers/conv.py::weight_scale bounds its exponent, to the range in which 2^e and 2^-e are both normal float32 numbers:
        // a channel whose largest weight is below 2^-113 (a dead BN gamma) keeps a finite scale and lands below 2^13 (e was up to 162:
        // 2^e = inf, the halves inf and NaN).  e >= -114 for every float32 amax, so the lower bound never acts.
        e = e > 126 ? 126 : (e < -126 ? -126 : e);
        const float sc = ldexpf(1.0f, e);
        out_scale[n] = ldexpf(1.0f, -e);
        for (int k = 0; k < MW_PITCH; ++k) {
            const int kh = k / 32, kc = k % 32;
            float v = 0.0f;
            if (k < 224 && kc < 21) v = host_weight_147x64[(kh * 21 + kc) * 64 + n] * sc;
            const _Float16 vh = (_Float16)v;
            hi[pos * MW_PITCH + k] = vh;
            lo[pos * MW_PITCH + k] = (_Float16)(v - (float)vh);
        }
    }
    return GPP_OK;
}

extern "C" int gpp_stem_conv7x7_bn_relu_x3(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                           int B, int H, int W, void* stream)
{
    return gpp_stem_conv7x7_bn_relu_x3_rc(in, packed_weight_x3, bias, out, B, H, W, nullptr, stream);
}

static int stem_x3_run(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                       int B, int H, int W, uint64_t* range_counter, const int32_t* heights, void* stream)
{
    if (!in || !packed_weight_x3 || !bias || !out || B <= 0 || H <= 0 || W <= 0) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)range_counter & 7) return GPP_ERR_ALIGN;
    if (((uintptr_t)out | (uintptr_t)packed_weight_x3) & 15) return GPP_ERR_ALIGN;
    constexpr int ROWS = 8;
    if (B > kMaxStemDim || H > kMaxStemDim || W > kMaxStemDim) return GPP_ERR_UNSUPPORTED;      // (the tile arithmetic below stays inside an int)
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    if ((int64_t)((Wo + TW - 1) / TW) * ((Ho + ROWS - 1) / ROWS) * B >= (1LL << 30)) return GPP_ERR_UNSUPPORTED;
    const int tiles = ((Wo + TW - 1) / TW) * ((Ho + ROWS - 1) / ROWS) * B;
    const int lds = 2 * 64 * MW_PITCH * 2 + 2 * (ROWS * 2 + 5) * MP_PITCH * 2;
    static std::atomic<unsigned long long> configured[2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return GPP_ERR_UNSUPPORTED;
    const int form = heights ? 1 : 0;
    if (!(configured[form].load(std::memory_order_acquire) >> dev & 1ull)) {
        hipError_t e = hipFuncSetAttribute(form ? (const void*)stem_mfma_x3_ragged_kernel<ROWS> : (const void*)stem_mfma_x3_kernel<ROWS>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        configured[form].fetch_or(1ull << dev, std::memory_order_release);
    }
    const unsigned grid = (unsigned)(tiles < 256 ? tiles : 256);                           // persistent workgroups, one per CU
    unsigned long long* counter = range_counter ? (unsigned long long*)range_counter : gpp_x3_range_counter_f16x3();   // (the library's: cached per device there)
    if (!counter) return GPP_ERR_UNSUPPORTED;
    if (heights)
        stem_mfma_x3_ragged_kernel<ROWS><<<grid, 64 * ROWS, lds, (hipStream_t)stream>>>(in, (const _Float16*)packed_weight_x3, bias, out, B, H, W, Ho, Wo, counter, heights);
    else
        stem_mfma_x3_kernel<ROWS><<<grid, 64 * ROWS, lds, (hipStream_t)stream>>>(in, (const _Float16*)packed_weight_x3, bias, out, B, H, W, Ho, Wo, counter);
    return result();
}

extern "C" int gpp_stem_conv7x7_bn_relu_x3_rc(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                              int B, int H, int W, uint64_t* range_counter, void* stream)
{
    return stem_x3_run(in, packed_weight_x3, bias, out, B, H, W, range_counter, nullptr, stream);
}

extern "C" int gpp_stem_conv7x7_bn_relu_x3_rc_ragged(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                                     int B, int H, int W, int Hp, const int32_t* heights, uint64_t* range_counter, void* stream)
{
    const int rc = ragged_check(heights, H, Hp, 4);
    return rc != GPP_OK ? rc : stem_x3_run(in, packed_weight_x3, bias, out, B, H, W, range_counter, heights, stream);
}

static int stem_mfma_run(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                         int dtype, int B, int H, int W, const int32_t* heights, void* stream)
{
    if (!in || !packed_weight_f16 || !bias || !out || B <= 0 || H <= 0 || W <= 0) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)out | (uintptr_t)packed_weight_f16) & 15) return GPP_ERR_ALIGN;
    if (B > kMaxStemDim || H > kMaxStemDim || W > kMaxStemDim) return GPP_ERR_UNSUPPORTED;      // (the tile arithmetic below stays inside an int)
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    if ((int64_t)((Wo + TW - 1) / TW) * ((Ho + TH - 1) / TH) * B >= (1LL << 30)) return GPP_ERR_UNSUPPORTED;
    const int tiles = ((Wo + TW - 1) / TW) * ((Ho + TH - 1) / TH) * B;
    static const int per_cu = [] { const char* e = getenv("GPP_STEM_WGS_PER_CU"); const int v = e ? atoi(e) : 2; return v < 1 ? 1 : (v > 4 ? 4 : v); }();
    const unsigned grid = (unsigned)(tiles < 256 * per_cu ? tiles : 256 * per_cu);      // persistent workgroups
    hipStream_t st = (hipStream_t)stream;
    if (dtype != GPP_BF16 && dtype != GPP_F16) return GPP_ERR_UNSUPPORTED;
    if (heights && dtype == GPP_BF16)
        stem_mfma_ragged_kernel<__bf16, bf16x8><<<grid, 256, 0, st>>>(in, (const _Float16*)packed_weight_f16, bias, (__bf16*)out, B, H, W, Ho, Wo, heights);
    else if (heights)
        stem_mfma_ragged_kernel<_Float16, f16x8><<<grid, 256, 0, st>>>(in, (const _Float16*)packed_weight_f16, bias, (_Float16*)out, B, H, W, Ho, Wo, heights);
    else if (dtype == GPP_BF16)
        stem_mfma_kernel<__bf16, bf16x8><<<grid, 256, 0, st>>>(in, (const _Float16*)packed_weight_f16, bias, (__bf16*)out, B, H, W, Ho, Wo);
    else
        stem_mfma_kernel<_Float16, f16x8><<<grid, 256, 0, st>>>(in, (const _Float16*)packed_weight_f16, bias, (_Float16*)out, B, H, W, Ho, Wo);
    return result();
}

extern "C" int gpp_stem_conv7x7_bn_relu_mfma(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                             int dtype, int B, int H, int W, void* stream)
{
    return stem_mfma_run(in, packed_weight_f16, bias, out, dtype, B, H, W, nullptr, stream);
}

extern "C" int gpp_stem_conv7x7_bn_relu_mfma_ragged(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                                    int dtype, int B, int H, int W, int Hp, const int32_t* heights, void* stream)
{
    const int rc = ragged_check(heights, H, Hp, 4);
    return rc != GPP_OK ? rc : stem_mfma_run(in, packed_weight_f16, bias, out, dtype, B, H, W, heights, stream);
}

static int stem_pool_mfma_run(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                              int dtype, int B, int H, int W, const int32_t* heights, void* stream)
{
    if (!in || !packed_weight_f16 || !bias || !out || B <= 0 || H <= 0 || W <= 0) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)out | (uintptr_t)packed_weight_f16) & 15) return GPP_ERR_ALIGN;
    if (dtype != GPP_BF16 && dtype != GPP_F16) return GPP_ERR_UNSUPPORTED;
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    const int Hp = (Ho + 1) / 2, Wp = (Wo + 1) / 2;
    const int pt = ((Hp - 1) * 2 + 3 - Ho > 0 ? (Hp - 1) * 2 + 3 - Ho : 0) / 2;
    const int pl = ((Wp - 1) * 2 + 3 - Wo > 0 ? (Wp - 1) * 2 + 3 - Wo : 0) / 2;
    // 8 conv rows per step, one workgroup per CU; GPP_STEM_POOL_ROWS=4: 4 rows, two workgroups per CU (measured equal:
    // 81 against 82 us at B = 8, 402 x 1333, tools/stem_time.py -- the kernel is bound by its LDS reads and patch loads, not by
    // the order of its phases)
    static const int rows = [] { const char* e = getenv("GPP_STEM_POOL_ROWS"); return (e && atoi(e) == 4) ? 4 : 8; }();
    const int pr = rows / 2;
    const int64_t total = (int64_t)B * ((Wp + FP_PCOLS - 1) / FP_PCOLS) * ((Hp + pr - 1) / pr);
    if (total >= (1LL << 30)) return GPP_ERR_UNSUPPORTED;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return GPP_ERR_UNSUPPORTED;
    const int64_t slots = (int64_t)cus * (8 / rows);                             // persistent workgroups
    const unsigned grid = (unsigned)(total < slots ? total : slots);
    hipStream_t st = (hipStream_t)stream;
    // hipFuncSetAttribute is per device: remember the devices each instantiation has been configured on
    static std::atomic<uint64_t> done[8];
    const int which = (dtype == GPP_BF16 ? 0 : 1) + (rows == 8 ? 0 : 2);
    const void* fns[8] = {(const void*)stem_pool_mfma_kernel<__bf16, bf16x8, 8>, (const void*)stem_pool_mfma_kernel<_Float16, f16x8, 8>,
                          (const void*)stem_pool_mfma_kernel<__bf16, bf16x8, 4>, (const void*)stem_pool_mfma_kernel<_Float16, f16x8, 4>,
                          (const void*)stem_pool_mfma_ragged_kernel<__bf16, bf16x8, 8>, (const void*)stem_pool_mfma_ragged_kernel<_Float16, f16x8, 8>,
                          (const void*)stem_pool_mfma_ragged_kernel<__bf16, bf16x8, 4>, (const void*)stem_pool_mfma_ragged_kernel<_Float16, f16x8, 4>};
    const int lds = fp_lds(rows);
    const int fn = which + (heights ? 4 : 0);
    if (!(done[fn].load(std::memory_order_acquire) & (1ull << (dev & 63)))) {
        const hipError_t e = hipFuncSetAttribute(fns[fn], hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        done[fn].fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
    const _Float16* wp = (const _Float16*)packed_weight_f16;
    if (heights) {
        if (which == 0) stem_pool_mfma_ragged_kernel<__bf16, bf16x8, 8><<<grid, 512, lds, st>>>(in, wp, bias, (__bf16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, heights);
        else if (which == 1) stem_pool_mfma_ragged_kernel<_Float16, f16x8, 8><<<grid, 512, lds, st>>>(in, wp, bias, (_Float16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, heights);
        else if (which == 2) stem_pool_mfma_ragged_kernel<__bf16, bf16x8, 4><<<grid, 256, lds, st>>>(in, wp, bias, (__bf16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, heights);
        else stem_pool_mfma_ragged_kernel<_Float16, f16x8, 4><<<grid, 256, lds, st>>>(in, wp, bias, (_Float16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, heights);
        return result();
    }
    if (which == 0) stem_pool_mfma_kernel<__bf16, bf16x8, 8><<<grid, 512, lds, st>>>(in, wp, bias, (__bf16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl);
    else if (which == 1) stem_pool_mfma_kernel<_Float16, f16x8, 8><<<grid, 512, lds, st>>>(in, wp, bias, (_Float16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl);
    else if (which == 2) stem_pool_mfma_kernel<__bf16, bf16x8, 4><<<grid, 256, lds, st>>>(in, wp, bias, (__bf16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl);
    else stem_pool_mfma_kernel<_Float16, f16x8, 4><<<grid, 256, lds, st>>>(in, wp, bias, (_Float16*)out, B, H, W, Ho, Wo, Hp, Wp, pt, pl);
    return result();
}

extern "C" int gpp_stem_pool_fused_mfma(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                        int dtype, int B, int H, int W, void* stream)
{
    return stem_pool_mfma_run(in, packed_weight_f16, bias, out, dtype, B, H, W, nullptr, stream);
}

extern "C" int gpp_stem_pool_fused_mfma_ragged(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                               int dtype, int B, int H, int W, int Hp, const int32_t* heights, void* stream)
{
    const int rc = ragged_check(heights, H, Hp, 4);
    return rc != GPP_OK ? rc : stem_pool_mfma_run(in, packed_weight_f16, bias, out, dtype, B, H, W, heights, stream);
}

static int stem_pool_x3_run(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                            int B, int H, int W, uint64_t* range_counter, const int32_t* heights, void* stream)
{
    if (!in || !packed_weight_x3 || !bias || !out || B <= 0 || H <= 0 || W <= 0) return GPP_ERR_BAD_ARG;
    if ((uintptr_t)range_counter & 7) return GPP_ERR_ALIGN;
    if (((uintptr_t)out | (uintptr_t)packed_weight_x3) & 15) return GPP_ERR_ALIGN;
    const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
    const int Hp = (Ho + 1) / 2, Wp = (Wo + 1) / 2;
    const int pt = ((Hp - 1) * 2 + 3 - Ho > 0 ? (Hp - 1) * 2 + 3 - Ho : 0) / 2;
    const int pl = ((Wp - 1) * 2 + 3 - Wo > 0 ? (Wp - 1) * 2 + 3 - Wo : 0) / 2;
    // 6 conv rows per step (6 wavefronts); GPP_STEM_POOL_X3_ROWS=4: 4.  One workgroup per CU either way (the hi / lo weights alone are 58 KB).
    // The ragged form always takes 4: the 6-wavefront kernel sits exactly at its 256 vector registers, and the per-image geometry costs
    // it four more (spilled to scratch, which tools/isa_audit.py refuses).
    static const int env_rows = [] { const char* e = getenv("GPP_STEM_POOL_X3_ROWS"); return (e && atoi(e) == 4) ? 4 : 6; }();
    const int rows = heights ? 4 : env_rows;
    const int pr = rows / 2;
    const int64_t total = (int64_t)B * ((Wp + FP_PCOLS - 1) / FP_PCOLS) * ((Hp + pr - 1) / pr);
    if (total >= (1LL << 30)) return GPP_ERR_UNSUPPORTED;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return GPP_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)(total < cus ? total : cus);                  // persistent workgroups
    hipStream_t st = (hipStream_t)stream;
    static std::atomic<uint64_t> done[4];
    const int which = rows == 6 ? 0 : 1;
    const void* fns[4] = {(const void*)stem_pool_mfma_x3_kernel<6>, (const void*)stem_pool_mfma_x3_kernel<4>,
                          nullptr, (const void*)stem_pool_mfma_x3_ragged_kernel<4>};
    const int lds = xp_lds(rows);
    const int fn = which + (heights ? 2 : 0);
    if (!(done[fn].load(std::memory_order_acquire) & (1ull << (dev & 63)))) {
        const hipError_t e = hipFuncSetAttribute(fns[fn], hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        done[fn].fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
    unsigned long long* counter = range_counter ? (unsigned long long*)range_counter : gpp_x3_range_counter_f16x3();
    if (!counter) return GPP_ERR_UNSUPPORTED;
    const _Float16* wp = (const _Float16*)packed_weight_x3;
    if (heights) stem_pool_mfma_x3_ragged_kernel<4><<<grid, 256, lds, st>>>(in, wp, bias, out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, counter, heights);
    else if (which == 0) stem_pool_mfma_x3_kernel<6><<<grid, 384, lds, st>>>(in, wp, bias, out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, counter);
    else stem_pool_mfma_x3_kernel<4><<<grid, 256, lds, st>>>(in, wp, bias, out, B, H, W, Ho, Wo, Hp, Wp, pt, pl, counter);
    return result();
}

extern "C" int gpp_stem_pool_fused_x3(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                      int B, int H, int W, uint64_t* range_counter, void* stream)
{
    return stem_pool_x3_run(in, packed_weight_x3, bias, out, B, H, W, range_counter, nullptr, stream);
}

extern "C" int gpp_stem_pool_fused_x3_ragged(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                             int B, int H, int W, int Hp, const int32_t* heights, uint64_t* range_counter, void* stream)
{
    const int rc = ragged_check(heights, H, Hp, 4);
    return rc != GPP_OK ? rc : stem_pool_x3_run(in, packed_weight_x3, bias, out, B, H, W, range_counter, heights, stream);
}

static int maxpool_run(const void* in, void* out, int dtype, int B, int H, int W, int C, const int32_t* heights, void* stream)
{
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)in | (uintptr_t)out) & 15) return GPP_ERR_ALIGN;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int pt = ((Ho - 1) * 2 + 3 - H > 0 ? (Ho - 1) * 2 + 3 - H : 0) / 2;
    const int pl = ((Wo - 1) * 2 + 3 - W > 0 ? (Wo - 1) * 2 + 3 - W : 0) / 2;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 8);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != GPP_BF16 && dtype != GPP_F16 && dtype != GPP_F32) return GPP_ERR_UNSUPPORTED;
    if (heights) {
        if (dtype == GPP_BF16)
            maxpool_ragged_kernel<__bf16, bf16x8><<<blocks, 256, 0, st>>>((const __bf16*)in, (__bf16*)out, B, H, W, C, Ho, Wo, pt, pl, heights);
        else if (dtype == GPP_F16)
            maxpool_ragged_kernel<_Float16, f16x8><<<blocks, 256, 0, st>>>((const _Float16*)in, (_Float16*)out, B, H, W, C, Ho, Wo, pt, pl, heights);
        else
            maxpool_ragged_kernel<float, f32x8><<<blocks, 256, 0, st>>>((const float*)in, (float*)out, B, H, W, C, Ho, Wo, pt, pl, heights);
        return result();
    }
    if (dtype == GPP_BF16)
        maxpool_kernel<__bf16, bf16x8><<<blocks, 256, 0, st>>>((const __bf16*)in, (__bf16*)out, B, H, W, C, Ho, Wo, pt, pl);
    else if (dtype == GPP_F16)
        maxpool_kernel<_Float16, f16x8><<<blocks, 256, 0, st>>>((const _Float16*)in, (_Float16*)out, B, H, W, C, Ho, Wo, pt, pl);
    else if (dtype == GPP_F32)
        maxpool_kernel<float, f32x8><<<blocks, 256, 0, st>>>((const float*)in, (float*)out, B, H, W, C, Ho, Wo, pt, pl);
    else
        return GPP_ERR_UNSUPPORTED;
    return result();
}

extern "C" int gpp_maxpool3x3s2_same(const void* in, void* out, int dtype, int B, int H, int W, int C, void* stream)
{
    return maxpool_run(in, out, dtype, B, H, W, C, nullptr, stream);
}

extern "C" int gpp_maxpool3x3s2_same_ragged(const void* in, void* out, int dtype, int B, int H, int W, int C, int Hp,
                                            const int32_t* heights, void* stream)
{
    const int rc = ragged_check(heights, H, Hp, 2);
    return rc != GPP_OK ? rc : maxpool_run(in, out, dtype, B, H, W, C, heights, stream);
}

extern "C" int gpp_relu_strided(const void* in, int64_t in_bstride, void* out, int64_t out_bstride, int dtype, int B,
                                int64_t count, void* stream)
{
    if (!in || !out || B <= 0 || count <= 0 || count % 8 != 0 || in_bstride % 8 != 0 || out_bstride % 8 != 0)
        return GPP_ERR_BAD_ARG;
    if (((uintptr_t)in | (uintptr_t)out) & 15) return GPP_ERR_ALIGN;
    const int64_t n8 = count / 8;
    const dim3 grid((unsigned)((n8 + 255) / 256 < 4096 ? (n8 + 255) / 256 : 4096), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == GPP_BF16X3 || dtype == GPP_F16X3) {      // a pre-split map (the sign bit of a half sits in the same place for both types)
        if (count % 32 != 0 || in_bstride % 32 != 0 || out_bstride % 32 != 0) return GPP_ERR_BAD_ARG;
        relu_x3_kernel<<<grid, 256, 0, st>>>((const char*)in, in_bstride * 4, (char*)out, out_bstride * 4, count / 8);
        return result();
    }
    if (dtype == GPP_BF16)
        relu_kernel<__bf16, bf16x8><<<grid, 256, 0, st>>>((const __bf16*)in, in_bstride, (__bf16*)out, out_bstride, n8);
    else if (dtype == GPP_F16)
        relu_kernel<_Float16, f16x8><<<grid, 256, 0, st>>>((const _Float16*)in, in_bstride, (_Float16*)out, out_bstride, n8);
    else if (dtype == GPP_F32)
        relu_kernel<float, f32x8><<<grid, 256, 0, st>>>((const float*)in, in_bstride, (float*)out, out_bstride, n8);
    else
        return GPP_ERR_UNSUPPORTED;
    return result();
}

extern "C" int gpp_relu(const void* in, void* out, int dtype, int64_t count, void* stream)
{
    return gpp_relu_strided(in, 0, out, 0, dtype, 1, count, stream);
}
