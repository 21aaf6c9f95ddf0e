// Instantiates the implicit-GEMM convolution kernels (conv_igemm_impl.h) for one element type: GPP_F32.
#include "conv_igemm_impl.h"
#include "conv_igemm_types.h"

int gpp_conv_dispatch_f32(gpp_conv_desc& d, hipStream_t st) { return dispatch<GPP_F32>(d, st); }

int gpp_preact_dispatch_f32(gpp_conv_desc& d, const float* in_scale, const float* in_shift, hipStream_t st)
{
    return dispatch_preact<GPP_F32>(d, in_scale, in_shift, st);
}
