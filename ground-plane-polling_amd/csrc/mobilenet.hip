// The MobileNet (v1) backbone of keras.applications.mobilenet.MobileNet(include_top=False): two kernels, float32 NHWC storage.
//
//   gpp_mobilenet_stem    conv1_pad ZeroPadding2D(1) + conv1 3x3 / 2 'valid' (3 -> C_out channels) + folded conv1_bn + ReLU6, a direct
//                         convolution on the vector ALUs: byte-bound (51 MB in, 137 MB out at B = 8, 402 x 1333), the same bytes in
//                         every arithmetic mode.
//   gpp_mobilenet_block   one depthwise-separable block as ONE launch: conv_pad_i ZeroPadding2D(1) + conv_dw_i 3x3 'valid' (stride 1
//                         or 2, depth multiplier 1) + folded BN + ReLU6, computed in float32 on the vector ALUs straight into the
//                         activation tile in LDS, K-chunk (32 channels) by K-chunk, then conv_pw_i 1x1 on the matrix pipe, folded BN bias
//                         + ReLU6 in the epilogue, float32 store through an output pitch.  The depthwise map never exists in HBM.
//
// Padding rule (ONE function: tap_origin): symmetric pad 1, so output (oy, ox) reads input rows oy * stride - 1 + dy, dy = 0..2 -- on an
// even side at stride 2 that is one pixel further up-left than TensorFlow's 'same' window.  H_out = (H - 1) / stride + 1.
//
// Arithmetic, in one documented order (this file is compiled with -ffp-contract=off: every multiply and add below rounds on its own, so
// a NumPy float32 loop in the same order gives the same bits):
//   depthwise  v = x(0,0) * w(0,0);  v = v + x(dy,dx) * w(dy,dx) for (dy, dx) = (0,1), (0,2), (1,0) .. (2,2);  v = v + bias;
//              v = min(max(v, 0), 6).  A tap that falls on the padding contributes the product 0 * w like any other tap.
//   stem       the same with 27 taps in (dy, dx, input channel) order.
//   pointwise  K (the input channel) runs in chunks of 32, chunk after chunk, zero-filled beyond C_in (both operands).
//              GPP_F32: v_mfma_f32_16x16x4_f32, a float32 fma chain; inside a chunk the channels run in the order
//              16 g + s + 4 q  (g = 0..1 outer, s = 0..3, q = 0..3 inner: q is the k index inside one instruction).
//              GPP_F16X3 / GPP_BF16X3: x = hi + lo and w = hi + lo (two 16-bit halves each), three v_mfma_f32_16x16x32 per chunk in
//              the order  w_lo x_hi,  w_hi x_lo,  w_hi x_hi.  The f16x3 weights carry a per-channel power of two whose inverse
//              (out_scale) multiplies the accumulator before the bias is added.  The depthwise result is at most 6, so its hi / lo
//              halves are always inside the IEEE-half range: this kernel needs no range counter.
//   epilogue   r = acc [* out_scale] ; r = r + bias ; r = min(max(r, 0), 6).
// An output element's K order and tap order are the same in every tile, so every tile choice gives the same bytes and an image's result
// does not depend on the batch it is in.  The block stores its output clamped: C3 / C4 / C5 as the FPN reads them are post-ReLU6 maps.
//
// Tiles: TM output pixels (linear over batch x H_out x W_out) x TN output channels per workgroup of four wavefronts; the depthwise
// values of a K-chunk are computed once per workgroup, so wide layers take wide tiles (64 x 256).  LDS rows are 128 bytes + 16 bytes of
// padding: the 16-byte fragment reads of 16 consecutive rows fall on 16 different bank groups.  At most 46 KiB of LDS per workgroup:
// three workgroups per CU.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gpp.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int KC = 32;            // channels per K-chunk: 128 bytes of float32, or [32 hi | 32 lo] 16-bit halves
constexpr int ROWB = 144;         // bytes of one LDS row: 128 + 16 of padding

enum { MODE_F32 = 0, MODE_F16X3 = 1, MODE_BF16X3 = 2 };

// the padding rule: first input row / column of the 3 x 3 window of output row / column o (ZeroPadding2D(1), then 'valid')
__host__ __device__ inline int tap_origin(int o, int stride) { return o * stride - 1; }
inline int out_size(int n, int stride) { return (n + 2 - 3) / stride + 1; }

struct BlockArgs {
    const float* in;
    const float* dw_w;            // [9][C_in], BN folded
    const float* dw_b;            // [C_in]
    const unsigned char* pw_w;    // [rows][k_chunks][128 bytes]
    const float* pw_b;            // [C_out]
    const float* out_scale;       // [C_out] (f16x3) or null
    float* out;
    int H, W, Ho, Wo, C_in, C_out, stride, in_pitch, out_pitch, k_chunks, n_tiles;
    int64_t total;                // B * Ho * Wo
};

__device__ __forceinline__ f32x4 relu6(f32x4 v)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fminf(fmaxf(v[k], 0.0f), 6.0f);
    return v;
}

template <int MODE, int GM, int GN, int WM, int WN>
__global__ __launch_bounds__(256) void mbn_block_kernel(const BlockArgs a)
{
    static_assert(GM * GN == 4, "four wavefronts");
    constexpr int TM = GM * WM * 16, TN = GN * WN * 16;
    constexpr int XI = TM / 32, WI = TN / 32;         // 16-byte items per thread: 8 per row, 256 threads
    __shared__ __attribute__((aligned(16))) unsigned char lds[(TM + TN) * ROWB];
    unsigned char* xs = lds;
    unsigned char* ws = lds + TM * ROWB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = (int)(blockIdx.x % (unsigned)a.n_tiles);
    const int64_t p0 = (int64_t)(blockIdx.x / (unsigned)a.n_tiles) * TM;
    const int n0 = nt * TN;
    const int wm = wave / GN, wn = wave % GN;
    const int cg = tid & 7, row = tid >> 3;

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the window of each of this thread's output pixels (the same for every K-chunk)
    const float* base[XI];
    int iy0[XI], ix0[XI];
    bool live[XI];
#pragma unroll
    for (int it = 0; it < XI; ++it) {
        const int64_t p = p0 + row + 32 * it;
        live[it] = p < a.total;
        const int64_t q = live[it] ? p : 0;
        const int ox = (int)(q % a.Wo);
        const int64_t r = q / a.Wo;
        const int oy = (int)(r % a.Ho);
        const int64_t b = r / a.Ho;
        base[it] = a.in + b * a.H * a.W * a.in_pitch;
        iy0[it] = tap_origin(oy, a.stride);
        ix0[it] = tap_origin(ox, a.stride);
    }

    for (int kc = 0; kc < a.k_chunks; ++kc) {
        __syncthreads();                               // the fragments of the chunk before have been read
        const int c = kc * KC + cg * 4;
        const bool cok = c < a.C_in;                   // (C_in % 4 == 0: four channels are inside or outside together)
        f32x4 w[9], wb;
        if (cok) {
#pragma unroll
            for (int t = 0; t < 9; ++t) w[t] = *(const f32x4*)(a.dw_w + (int64_t)t * a.C_in + c);
            wb = *(const f32x4*)(a.dw_b + c);
        }
#pragma unroll
        for (int it = 0; it < XI; ++it) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (cok && live[it]) {
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int iy = iy0[it] + dy, ix = ix0[it] + dx;
                        f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
                        if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                            x = *(const f32x4*)(base[it] + ((int64_t)iy * a.W + ix) * a.in_pitch + c);
                        const f32x4 prod = x * w[dy * 3 + dx];
                        v = (dy == 0 && dx == 0) ? prod : v + prod;
                    }
                }
                v = relu6(v + wb);
            }
            unsigned char* dst = xs + (row + 32 * it) * ROWB;
            if constexpr (MODE == MODE_F32) {
                *(f32x4*)(dst + cg * 16) = v;
            } else if constexpr (MODE == MODE_F16X3) {
                f16x4 hi, lo;
#pragma unroll
                for (int k = 0; k < 4; ++k) { hi[k] = (_Float16)v[k]; lo[k] = (_Float16)(v[k] - (float)hi[k]); }
                *(f16x4*)(dst + cg * 8) = hi;
                *(f16x4*)(dst + 64 + cg * 8) = lo;
            } else {
                bf16x4 hi, lo;
#pragma unroll
                for (int k = 0; k < 4; ++k) { hi[k] = (__bf16)v[k]; lo[k] = (__bf16)(v[k] - (float)hi[k]); }
                *(bf16x4*)(dst + cg * 8) = hi;
                *(bf16x4*)(dst + 64 + cg * 8) = lo;
            }
        }
        // the weight rows of this chunk (the packed tensor has rows up to a multiple of 256 and k_chunks chunks: always in bounds)
#pragma unroll
        for (int it = 0; it < WI; ++it) {
            const int r = row + 32 * it;
            *(f32x4*)(ws + r * ROWB + cg * 16) = *(const f32x4*)(a.pw_w + ((int64_t)(n0 + r) * a.k_chunks + kc) * 128 + cg * 16);
        }
        __syncthreads();

        const unsigned char* xr = xs + (wm * WM * 16 + (lane & 15)) * ROWB + (lane >> 4) * 16;
        const unsigned char* wr = ws + (wn * WN * 16 + (lane & 15)) * ROWB + (lane >> 4) * 16;
        if constexpr (MODE == MODE_F32) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                f32x4 xf[WM], wf[WN];
#pragma unroll
                for (int i = 0; i < WM; ++i) xf[i] = *(const f32x4*)(xr + i * 16 * ROWB + g * 64);
#pragma unroll
                for (int j = 0; j < WN; ++j) wf[j] = *(const f32x4*)(wr + j * 16 * ROWB + g * 64);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < WM; ++i)
#pragma unroll
                        for (int j = 0; j < WN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j][s], xf[i][s], acc[i][j], 0, 0, 0);
            }
        } else if constexpr (MODE == MODE_F16X3) {
            f16x8 xh[WM], xl[WM], wh[WN], wl[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) { xh[i] = *(const f16x8*)(xr + i * 16 * ROWB); xl[i] = *(const f16x8*)(xr + i * 16 * ROWB + 64); }
#pragma unroll
            for (int j = 0; j < WN; ++j) { wh[j] = *(const f16x8*)(wr + j * 16 * ROWB); wl[j] = *(const f16x8*)(wr + j * 16 * ROWB + 64); }
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j], xh[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xl[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j], xh[i], acc[i][j], 0, 0, 0);
        } else {
            bf16x8 xh[WM], xl[WM], wh[WN], wl[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) { xh[i] = *(const bf16x8*)(xr + i * 16 * ROWB); xl[i] = *(const bf16x8*)(xr + i * 16 * ROWB + 64); }
#pragma unroll
            for (int j = 0; j < WN; ++j) { wh[j] = *(const bf16x8*)(wr + j * 16 * ROWB); wl[j] = *(const bf16x8*)(wr + j * 16 * ROWB + 64); }
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], xh[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xl[i], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xh[i], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: the accumulator holds output channels n .. n + 3 (rows of the instruction) of pixel lane & 15 (its column)
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int64_t p = p0 + wm * WM * 16 + i * 16 + (lane & 15);
        if (p >= a.total) continue;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int n = n0 + wn * WN * 16 + j * 16 + (lane >> 4) * 4;
            if (n >= a.C_out) continue;                // (C_out % 4 == 0)
            f32x4 r = acc[i][j];
            if constexpr (MODE == MODE_F16X3) r = r * *(const f32x4*)(a.out_scale + n);
            r = relu6(r + *(const f32x4*)(a.pw_b + n));
            *(f32x4*)(a.out + p * a.out_pitch + n) = r;
        }
    }
}

__global__ __launch_bounds__(256) void mbn_stem_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int B, int H, int W, int Ho, int Wo, int C, int out_pitch)
{
    const int cv = C / 4;
    const int64_t total = (int64_t)B * Ho * Wo * cv;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % cv) * 4;
        int64_t p = e / cv;
        const int ox = (int)(p % Wo);
        const int64_t r = p / Wo;
        const int oy = (int)(r % Ho);
        const int64_t b = r / Ho;
        const float* src = in + b * H * W * 3;
        const int iy0 = tap_origin(oy, 2), ix0 = tap_origin(ox, 2);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = iy0 + dy, ix = ix0 + dx;
                const bool inside = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const float* px = src + ((int64_t)iy * W + ix) * 3;
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const int t = (dy * 3 + dx) * 3 + ci;
                    const float x = inside ? px[ci] : 0.0f;
                    const f32x4 prod = x * *(const f32x4*)(w + t * C + c);
                    v = t == 0 ? prod : v + prod;
                }
            }
        }
        v = relu6(v + *(const f32x4*)(bias + c));
        *(f32x4*)(out + p * out_pitch + c) = v;
    }
}

// the depthwise half of a block on its own, its map stored to HBM: NOT a product path -- tools/bench_mobilenet.py times it (plus a plain
// 1 x 1 convolution) against the fused launch.  The same arithmetic as the fused kernel's first half.
__global__ __launch_bounds__(256) void mbn_depthwise_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out, int B, int H, int W, int Ho, int Wo, int C, int stride,
                                                            int in_pitch, int out_pitch)
{
    const int cv = C / 4;
    const int64_t total = (int64_t)B * Ho * Wo * cv;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % cv) * 4;
        const int64_t p = e / cv;
        const int ox = (int)(p % Wo);
        const int64_t r = p / Wo;
        const int oy = (int)(r % Ho);
        const int64_t b = r / Ho;
        const float* src = in + b * H * W * in_pitch + c;
        const int iy0 = tap_origin(oy, stride), ix0 = tap_origin(ox, stride);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = iy0 + dy, ix = ix0 + dx;
                f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) x = *(const f32x4*)(src + ((int64_t)iy * W + ix) * in_pitch);
                const f32x4 prod = x * *(const f32x4*)(w + (dy * 3 + dx) * C + c);
                v = (dy == 0 && dx == 0) ? prod : v + prod;
            }
        }
        *(f32x4*)(out + p * out_pitch + c) = relu6(v + *(const f32x4*)(bias + c));
    }
}

const int kBlockTiles[] = {0, 128064, 64128, 128128, 64256};

int default_tile(const gpp_mobilenet_block_desc& d) { return d.C_out <= 64 ? 128064 : d.C_out <= 128 ? 128128 : 64256; }

void tile_dims(int tile, int& tm, int& tn) { tm = tile / 1000; tn = tile % 1000; }

int validate(const gpp_mobilenet_block_desc& d)
{
    if (!d.in || !d.dw_weight || !d.dw_bias || !d.pw_weight || !d.pw_bias || !d.out) return GPP_ERR_BAD_ARG;
    if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.C_in <= 0 || d.C_out <= 0) return GPP_ERR_BAD_ARG;
    if (d.C_in % 4 != 0 || d.C_out % 4 != 0 || d.in_pitch < d.C_in || d.in_pitch % 4 != 0 || d.out_pitch < d.C_out || d.out_pitch % 4 != 0)
        return GPP_ERR_BAD_ARG;
    if (d.stride != 1 && d.stride != 2) return GPP_ERR_UNSUPPORTED;
    if (d.dtype != GPP_F32 && d.dtype != GPP_F16X3 && d.dtype != GPP_BF16X3) return GPP_ERR_UNSUPPORTED;
    if (d.reserved != 0) return GPP_ERR_BAD_ARG;
    if (d.C_in > 8192 || d.C_out > 8192) return GPP_ERR_UNSUPPORTED;
    if (d.weight_rows < d.C_out || d.weight_rows % 256 != 0) return GPP_ERR_BAD_ARG;       // (every tile reads whole rows of zeros beyond C_out)
    if (d.dtype == GPP_F16X3 && !d.out_scale) return GPP_ERR_BAD_ARG;
    if ((int64_t)d.B * d.H * d.W * d.in_pitch >= (1LL << 40)) return GPP_ERR_UNSUPPORTED;
    if ((int64_t)d.B * out_size(d.H, d.stride) * out_size(d.W, d.stride) * d.out_pitch >= (1LL << 40)) return GPP_ERR_UNSUPPORTED;
    if (((uintptr_t)d.in | (uintptr_t)d.dw_weight | (uintptr_t)d.dw_bias | (uintptr_t)d.pw_weight | (uintptr_t)d.pw_bias |
         (uintptr_t)d.out_scale | (uintptr_t)d.out) & 15)
        return GPP_ERR_ALIGN;
    bool listed = false;
    for (int t : kBlockTiles) listed = listed || t == d.tile_hint;
    if (!listed) return GPP_ERR_BAD_ARG;
    return GPP_OK;
}

template <int MODE, int GM, int GN, int WM, int WN>
int launch_tile(const BlockArgs& a, hipStream_t st)
{
    constexpr int TM = GM * WM * 16;
    const int64_t blocks = (a.total + TM - 1) / TM * a.n_tiles;
    if (blocks > 0x7fffffffLL) return GPP_ERR_UNSUPPORTED;
    mbn_block_kernel<MODE, GM, GN, WM, WN><<<(unsigned)blocks, 256, 0, st>>>(a);
    return (int)hipGetLastError();
}

template <int MODE>
int launch_mode(BlockArgs& a, int tile, hipStream_t st)
{
    int tm, tn;
    tile_dims(tile, tm, tn);
    a.n_tiles = (a.C_out + tn - 1) / tn;
    switch (tile) {
        case 128064: return launch_tile<MODE, 4, 1, 2, 4>(a, st);
        case 64128: return launch_tile<MODE, 2, 2, 2, 4>(a, st);
        case 128128: return launch_tile<MODE, 2, 2, 4, 4>(a, st);
        case 64256: return launch_tile<MODE, 1, 4, 4, 4>(a, st);
        default: return GPP_ERR_BAD_ARG;
    }
}

}  // namespace

extern "C" int gpp_mobilenet_block(const gpp_mobilenet_block_desc* desc, void* stream)
{
    if (!desc) return GPP_ERR_BAD_ARG;
    const gpp_mobilenet_block_desc d = *desc;
    const int rc = validate(d);
    if (rc != GPP_OK) return rc;
    BlockArgs a;
    a.in = d.in; a.dw_w = d.dw_weight; a.dw_b = d.dw_bias; a.pw_w = (const unsigned char*)d.pw_weight; a.pw_b = d.pw_bias;
    a.out_scale = d.out_scale; a.out = d.out;
    a.H = d.H; a.W = d.W; a.Ho = out_size(d.H, d.stride); a.Wo = out_size(d.W, d.stride);
    a.C_in = d.C_in; a.C_out = d.C_out; a.stride = d.stride; a.in_pitch = d.in_pitch; a.out_pitch = d.out_pitch;
    a.k_chunks = (d.C_in + KC - 1) / KC;
    a.n_tiles = 1;
    a.total = (int64_t)d.B * a.Ho * a.Wo;
    const int tile = d.tile_hint ? d.tile_hint : default_tile(d);
    hipStream_t st = (hipStream_t)stream;
    switch (d.dtype) {
        case GPP_F16X3: return launch_mode<MODE_F16X3>(a, tile, st);
        case GPP_BF16X3: return launch_mode<MODE_BF16X3>(a, tile, st);
        default: return launch_mode<MODE_F32>(a, tile, st);
    }
}

extern "C" int gpp_mobilenet_block_tile_candidates(const gpp_mobilenet_block_desc* desc, int* tiles, int capacity, int* count)
{
    if (!desc || !count || capacity < 0 || (capacity > 0 && !tiles)) return GPP_ERR_BAD_ARG;
    gpp_mobilenet_block_desc d = *desc;
    d.tile_hint = 0;
    const int rc = validate(d);
    if (rc != GPP_OK) return rc;
    int n = 0;
    for (int tile : kBlockTiles) {
        if (n < capacity) tiles[n] = tile;
        ++n;
    }
    *count = n;
    return GPP_OK;
}

extern "C" int gpp_mobilenet_block_autotune(gpp_mobilenet_block_desc* desc, int iters, void* stream, float* best_us)
{
    if (!desc || iters < 1) return GPP_ERR_BAD_ARG;
    {
        gpp_mobilenet_block_desc d = *desc;
        d.tile_hint = 0;
        const int rc = validate(d);
        if (rc != GPP_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    hipError_t e = hipEventCreate(&e0);
    if (e != hipSuccess) return (int)e;
    e = hipEventCreate(&e1);
    if (e != hipSuccess) { (void)hipEventDestroy(e0); return (int)e; }
    const int tile_in = desc->tile_hint;
    float best = 1e30f;
    int best_tile = tile_in, rc = GPP_OK;
    for (int tile : kBlockTiles) {
        desc->tile_hint = tile;
        int r = gpp_mobilenet_block(desc, stream);             // warm-up
        if (r != GPP_OK) { rc = r; break; }
        float t_best = 1e30f;
        for (int rep = 0; rep < 2 && r == GPP_OK; ++rep) {
            (void)hipEventRecord(e0, st);
            for (int i = 0; i < iters; ++i) (void)gpp_mobilenet_block(desc, stream);
            (void)hipEventRecord(e1, st);
            const hipError_t s = hipEventSynchronize(e1);
            if (s != hipSuccess) { r = (int)s; break; }
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            t_best = ms < t_best ? ms : t_best;
        }
        if (r != GPP_OK) { rc = r; break; }
        const float us = t_best * 1000.0f / iters;
        if (us < best) { best = us; best_tile = tile; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    desc->tile_hint = rc == GPP_OK ? best_tile : tile_in;
    if (best_us) *best_us = best;
    return rc;
}

extern "C" int gpp_mobilenet_stem(const float* in, const float* weight, const float* bias, float* out, int B, int H, int W, int C_out,
                                  int out_pitch, void* stream)
{
    if (!in || !weight || !bias || !out || B <= 0 || H <= 0 || W <= 0 || C_out <= 0 || C_out % 4 != 0 || out_pitch < C_out || out_pitch % 4 != 0)
        return GPP_ERR_BAD_ARG;
    if (C_out > 1024) return GPP_ERR_UNSUPPORTED;
    if ((int64_t)B * H * W * 3 >= (1LL << 40) || (int64_t)B * out_size(H, 2) * out_size(W, 2) * out_pitch >= (1LL << 40)) return GPP_ERR_UNSUPPORTED;
    if (((uintptr_t)in | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)out) & 15) return GPP_ERR_ALIGN;
    const int Ho = out_size(H, 2), Wo = out_size(W, 2);
    const int64_t total = (int64_t)B * Ho * Wo * (C_out / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    mbn_stem_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(in, weight, bias, out, B, H, W, Ho, Wo, C_out, out_pitch);
    return (int)hipGetLastError();
}

extern "C" int gpp_mobilenet_depthwise(const float* in, const float* weight, const float* bias, float* out, int B, int H, int W, int C, int stride,
                                       int in_pitch, int out_pitch, void* stream)
{
    if (!in || !weight || !bias || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || in_pitch < C || in_pitch % 4 != 0 ||
        out_pitch < C || out_pitch % 4 != 0)
        return GPP_ERR_BAD_ARG;
    if (stride != 1 && stride != 2) return GPP_ERR_UNSUPPORTED;
    if ((int64_t)B * H * W * in_pitch >= (1LL << 40) || (int64_t)B * out_size(H, stride) * out_size(W, stride) * out_pitch >= (1LL << 40))
        return GPP_ERR_UNSUPPORTED;
    if (((uintptr_t)in | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)out) & 15) return GPP_ERR_ALIGN;
    const int Ho = out_size(H, stride), Wo = out_size(W, stride);
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    mbn_depthwise_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(in, weight, bias, out, B, H, W, Ho, Wo, C, stride, in_pitch, out_pitch);
    return (int)hipGetLastError();
}
