// Instantiates the gathered-row form of the implicit-GEMM convolution (conv_igemm_impl.h: GATHER) for every element type: the head
// output layers evaluated on the pixels the decode reads (gpp_conv_desc.gather_rows).
#include "conv_igemm_impl.h"
#include "conv_igemm_types.h"

int gpp_conv_gather_dispatch(gpp_conv_desc& d, hipStream_t st)
{
    switch (d.dtype) {
        case GPP_BF16: return dispatch_gather<GPP_BF16>(d, st);
        case GPP_F16: return dispatch_gather<GPP_F16>(d, st);
        case GPP_BF16X3: return dispatch_gather<GPP_BF16X3>(d, st);
        case GPP_F16X3: return dispatch_gather<GPP_F16X3>(d, st);
        default: return dispatch_gather<GPP_F32>(d, st);
    }
}
