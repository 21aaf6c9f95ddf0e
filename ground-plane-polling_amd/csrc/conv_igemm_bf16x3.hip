// Instantiates the implicit-GEMM convolution kernels (conv_igemm_impl.h) for one element type: GPP_BF16X3
// (float32 storage, three bf16 matrix products per float32 product).
#include "conv_igemm_impl.h"
#include "conv_igemm_types.h"

int gpp_conv_dispatch_bf16x3(gpp_conv_desc& d, hipStream_t st) { return dispatch<GPP_BF16X3>(d, st); }

int gpp_preact_dispatch_bf16x3(gpp_conv_desc& d, const float* in_scale, const float* in_shift, hipStream_t st)
{
    return dispatch_preact<GPP_BF16X3>(d, in_scale, in_shift, st);
}

int gpp_tail_dispatch_bf16x3(gpp_conv_desc& d1, gpp_conv_desc& d2, int tile_rows, hipStream_t st)
{
    return dispatch_tail_x3<GPP_BF16X3>(d1, d2, tile_rows, st);
}
