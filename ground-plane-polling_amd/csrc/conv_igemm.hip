// C ABI of the implicit-GEMM convolution (include/gpp.h): argument validation, the batch-independent split-K rule,
// dispatch to the per-element-type kernels (conv_igemm_{bf16,f16,f32}.hip <- conv_igemm_impl.h) and the tile autotuner.
//
// Replaces the Conv2D / BatchNormalization(frozen) / Activation / Add / UpsampleLike nodes of
//   /root/reference/keras_retinanet_3D/models/retinanet.py:24-205  (heads, FPN)
//   keras_resnet bottleneck stack used at models/resnet.py:88-93     (third party)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "conv_igemm_types.h"
#include "conv_tiles.h"
#include "gpp.h"

namespace {

inline bool is_x3(int dtype) { return dtype == GPP_BF16X3 || dtype == GPP_F16X3; }
inline bool f32_storage(int dtype) { return dtype == GPP_F32 || is_x3(dtype); }
inline int elem_size(int dtype) { return f32_storage(dtype) ? 4 : 2; }

int validate(const gpp_conv_desc& d)
{
    if (!d.in || !d.weight || !d.out) return GPP_ERR_BAD_ARG;
    if (d.dtype != GPP_BF16 && d.dtype != GPP_F16 && d.dtype != GPP_F32 && !is_x3(d.dtype)) return GPP_ERR_UNSUPPORTED;
    const int esz = elem_size(d.dtype), ck = 128 / esz, va = 16 / esz;     // channels per K-step, elements per 16 bytes
    if (d.batch <= 0 || d.C_in <= 0 || d.C_out <= 0 || d.KH <= 0 || d.KW <= 0) return GPP_ERR_BAD_ARG;
    // sizes beyond anything a 2 GiB map can hold: refused here, so that the 64-bit size arithmetic below and in the launchers cannot overflow
    constexpr int kMaxDim = 1 << 20;
    if (d.batch > kMaxDim || d.C_in > kMaxDim || d.C_out > kMaxDim || d.in_pitch > kMaxDim || d.out_pitch > kMaxDim || d.res_pitch > kMaxDim ||
        d.weight_rows > kMaxDim || d.weight_rows < 0 || d.in_pitch < 0 || d.out_pitch < 0 || d.res_pitch < 0 || d.partial_bytes < 0)
        return GPP_ERR_UNSUPPORTED;
    if (d.KH > 8 || d.KW > 8) return GPP_ERR_UNSUPPORTED;           // tap validity masks are 8 + 8 bits
    if (d.C_in % ck != 0 || d.C_out % 4 != 0) return GPP_ERR_UNSUPPORTED;
    if (d.stride != 1 && d.stride != 2) return GPP_ERR_UNSUPPORTED;
    if (d.n_groups < 1 || d.n_groups > GPP_MAX_GROUPS) return GPP_ERR_BAD_ARG;
    if (d.split_k < 0) return GPP_ERR_BAD_ARG;
#ifndef GPP_STAMPS
    if (d.reserved != 0) return GPP_ERR_BAD_ARG;                    // diagnostic switches exist in -DGPP_STAMPS builds only
#endif
    if (d.reserved2 != 0 || (d.x3_split & ~(GPP_X3_IN | GPP_X3_OUT | GPP_X3_RES))) return GPP_ERR_BAD_ARG;
    if (d.reserved3 != 0 || d.reserved4 != 0 || (d.gather_rows != nullptr) != (d.gather_counts != nullptr)) return GPP_ERR_BAD_ARG;
    // both forms behind one call (tower_rows / tower_counts / tower_flag): all three or none, and neither a list nor a guard of the caller's
    const bool tower = d.tower_rows || d.tower_counts || d.tower_flag;
    if (tower && (!d.tower_rows || !d.tower_counts || !d.tower_flag || d.gather_rows || d.guard)) return GPP_ERR_BAD_ARG;
    if (!tower && d.tower_tile != 0) return GPP_ERR_BAD_ARG;
    // the same pair for a layer further up the tower (deep_rows / deep_counts / deep_flag): the same rules, and never both sets
    const bool deep = d.deep_rows || d.deep_counts || d.deep_flag;
    if (deep && (!d.deep_rows || !d.deep_counts || !d.deep_flag || d.gather_rows || d.guard || tower)) return GPP_ERR_BAD_ARG;
    if (!deep && d.deep_tile != 0) return GPP_ERR_BAD_ARG;
    if (d.lists_after < 0) return GPP_ERR_BAD_ARG;
    // conv_after: a layer enqueued behind this one (and behind its lists) -- this one is then a plain dense launch, as the deep layers' rules go
    // conv_before: the same kind of handle in front of a plain dense call, which reads every row of the layer the handle names
    if (d.conv_after < 0 || d.conv_before < 0) return GPP_ERR_BAD_ARG;
    if ((d.conv_after || d.conv_before) && (d.gather_rows || d.guard || tower || deep)) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)d.gather_rows | (uintptr_t)d.gather_counts | (uintptr_t)d.guard | (uintptr_t)d.tower_rows | (uintptr_t)d.tower_counts |
         (uintptr_t)d.tower_flag | (uintptr_t)d.deep_rows | (uintptr_t)d.deep_counts | (uintptr_t)d.deep_flag) & 3)
        return GPP_ERR_ALIGN;
    // the gathered-row form: stride 1, no shortcut, never split (split-K would change the summation order of a row); float32 output, or -- a
    // layer between two convolutions -- the pre-split maps of an x3 type with whole 256-column tiles (gpp_tiles::gather_pipe_can_run)
    if (d.gather_rows && (d.stride != 1 || d.residual || d.split_k > 1)) return GPP_ERR_UNSUPPORTED;
    if (((d.gather_rows && !d.out_f32) || tower || deep) && !gpp_tiles::gather_pipe_can_run(d)) return GPP_ERR_UNSUPPORTED;
    if (d.x3_split && !is_x3(d.dtype)) return GPP_ERR_BAD_ARG;
    if (d.out_scale && d.dtype != GPP_F16X3) return GPP_ERR_BAD_ARG;
    if ((d.x3_split & GPP_X3_OUT) && (d.out_f32 || d.C_out % 32 != 0 || d.out_pitch % 32 != 0)) return GPP_ERR_UNSUPPORTED;
    if ((d.x3_split & GPP_X3_IN) && d.in_pitch % 32 != 0) return GPP_ERR_UNSUPPORTED;
    if ((d.x3_split & GPP_X3_RES) && (!d.residual || d.res_pitch % 32 != 0)) return GPP_ERR_UNSUPPORTED;
    const int oa = (d.out_f32 || f32_storage(d.dtype)) ? 4 : 8;        // output elements per 16 bytes
    if (d.in_pitch < d.C_in || d.in_pitch % va != 0) return GPP_ERR_ALIGN;
    if (d.out_pitch < d.C_out || d.out_pitch % oa != 0) return GPP_ERR_ALIGN;
    if (d.residual && (d.res_pitch < d.C_out || d.res_pitch % va != 0)) return GPP_ERR_ALIGN;
    if (((uintptr_t)d.in | (uintptr_t)d.weight | (uintptr_t)d.out | (uintptr_t)d.zero_page | (uintptr_t)d.residual |
         (uintptr_t)d.bias | (uintptr_t)d.partial) & 15)
        return GPP_ERR_ALIGN;
    for (int g = 0; g < d.n_groups; ++g) {
        const gpp_conv_group& G = d.groups[g];
        if (G.H_in <= 0 || G.W_in <= 0 || G.H_out <= 0 || G.W_out <= 0) return GPP_ERR_BAD_ARG;
        if (G.H_in > kMaxDim || G.W_in > kMaxDim || G.H_out > kMaxDim || G.W_out > kMaxDim || G.H_res > kMaxDim || G.W_res > kMaxDim) return GPP_ERR_UNSUPPORTED;
        constexpr int64_t kMaxOff = (int64_t)1 << 40;              // element offsets / image strides: far beyond any real buffer, far below overflow
        if (G.in_off < 0 || G.out_off < 0 || G.res_off < 0 || G.in_bstride < 0 || G.out_bstride < 0 || G.res_bstride < 0 || G.in_off > kMaxOff ||
            G.out_off > kMaxOff || G.res_off > kMaxOff || G.in_bstride > kMaxOff || G.out_bstride > kMaxOff || G.res_bstride > kMaxOff)
            return GPP_ERR_BAD_ARG;
        if ((G.out_off | G.out_bstride) % oa != 0) return GPP_ERR_ALIGN;
        if ((G.in_off | G.in_bstride) % va != 0) return GPP_ERR_ALIGN;
        if (d.residual && ((G.res_off | G.res_bstride) % va != 0 || G.H_res <= 0 || G.W_res <= 0)) return GPP_ERR_ALIGN;
        if ((int64_t)d.batch * G.H_out * G.W_out >= (1LL << 31)) return GPP_ERR_UNSUPPORTED;
        if ((d.x3_split & GPP_X3_OUT) && ((G.out_off | G.out_bstride) % 32 != 0)) return GPP_ERR_ALIGN;      // pre-split maps: whole 32-channel blocks
        if ((d.x3_split & GPP_X3_IN) && ((G.in_off | G.in_bstride) % 32 != 0)) return GPP_ERR_ALIGN;
        if ((d.x3_split & GPP_X3_RES) && ((G.res_off | G.res_bstride) % 32 != 0)) return GPP_ERR_ALIGN;
    }
    return GPP_OK;
}

// Split-K factor of a layer as a function of the LAYER ALONE -- kernel size, channels, output pixels PER IMAGE -- never of
// the batch size, the tile or a timing: the float32 summation order of an output element, and with it every bit of the
// result, is then the same whether an image is computed alone, in a batch of 64 or on another rank.
// Deep-K layers whose per-image tile grid is tiny (res5 branch2b, P5, P6, P7) are split; everything else is not.
int split_rule(const gpp_conv_desc& d)
{
    if (!d.partial) return 1;
    int64_t pix = 0;
    for (int g = 0; g < d.n_groups; ++g) pix += (int64_t)d.groups[g].H_out * d.groups[g].W_out;
    const int64_t tiles_per_image = ((pix + 127) / 128) * ((d.C_out + 127) / 128);
    const int64_t kdepth = (int64_t)d.KH * d.KW * d.C_in;
    if (tiles_per_image > 24 || kdepth < 3072) return 1;
    int split = (int)((kdepth + 768) / 1536);
    return split < 1 ? 1 : (split > 8 ? 8 : split);
}

// GPP_F16X3: a launch whose caller named no range counter adds to the library's per-device one
int fill_range_counter(gpp_conv_desc& d)
{
    if (d.dtype != GPP_F16X3) return d.range_counter ? GPP_ERR_BAD_ARG : GPP_OK;
    if (!d.range_counter) d.range_counter = (uint64_t*)gpp_x3_range_counter_f16x3();
    if (!d.range_counter) return GPP_ERR_UNSUPPORTED;
    return ((uintptr_t)d.range_counter & 7) ? GPP_ERR_ALIGN : GPP_OK;
}

int dispatch_any(gpp_conv_desc& d, hipStream_t st)
{
    const int rc = fill_range_counter(d);
    if (rc != GPP_OK) return rc;
    if (d.split_k == 0) d.split_k = split_rule(d);
    if (d.gather_rows) {
        // a layer the rule splits has another summation order than one gathered launch can give: refused, never computed differently
        if (d.split_k > 1) return GPP_ERR_UNSUPPORTED;
        return gpp_conv_gather_dispatch(d, st);
    }
    if (d.tower_rows || d.deep_rows) {
        // both forms on the stream, the device word chooses: the gathered launch works while it is 0, the dense one while it is 1 (the guard
        // mechanism of the head output layers, here behind one call: the plan keeps ONE op for the layer).  tower_* and deep_* name the
        // lists of two different writers (validate: never both); what is launched is the same
        if (d.split_k > 1) return GPP_ERR_UNSUPPORTED;
        const int32_t* flag = d.tower_rows ? d.tower_flag : d.deep_flag;
        gpp_conv_desc rows = d, dense = d;
        rows.gather_rows = d.tower_rows ? d.tower_rows : d.deep_rows;
        rows.gather_counts = d.tower_rows ? d.tower_counts : d.deep_counts;
        rows.tile_hint = d.tower_rows ? d.tower_tile : d.deep_tile;
        rows.guard = flag; rows.guard_value = 0;
        dense.guard = flag; dense.guard_value = 1;
        rows.tower_rows = rows.tower_counts = rows.tower_flag = dense.tower_rows = dense.tower_counts = dense.tower_flag = nullptr;
        rows.deep_rows = rows.deep_counts = rows.deep_flag = dense.deep_rows = dense.deep_counts = dense.deep_flag = nullptr;
        rows.tower_tile = dense.tower_tile = rows.deep_tile = dense.deep_tile = 0;
        const int rc_rows = gpp_conv_gather_dispatch(rows, st);
        if (rc_rows != GPP_OK) return rc_rows;
        return dispatch_any(dense, st);
    }
    switch (d.dtype) {
        case GPP_BF16: return gpp_conv_dispatch_bf16(d, st);
        case GPP_F16: return gpp_conv_dispatch_f16(d, st);
        case GPP_BF16X3: return gpp_conv_dispatch_bf16x3(d, st);
        case GPP_F16X3: return gpp_conv_dispatch_f16x3(d, st);
        default: return gpp_conv_dispatch_f32(d, st);
    }
}

int tail_entry(const gpp_conv_desc* conv3x3, const gpp_conv_desc* conv1x1, int tile_rows, void* stream)
{
    if (!conv3x3 || !conv1x1) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d1 = *conv3x3, d2 = *conv1x1;
    int rc = validate(d1);
    if (rc == GPP_OK) rc = validate(d2);
    if (rc != GPP_OK) return rc;
    if (d1.gather_rows || d2.gather_rows || d1.guard || d2.guard || d1.tower_rows || d2.tower_rows || d1.deep_rows || d2.deep_rows ||
        d1.lists_after || d2.lists_after || d1.conv_after || d2.conv_after || d1.conv_before || d2.conv_before)
        return GPP_ERR_UNSUPPORTED;      // gpp_conv2d_igemm only
    const gpp_conv_group &G1 = d1.groups[0], &G2 = d2.groups[0];
    // the pair this kernel fuses: 3x3 / stride 1 / pad 1 / C -> C (C = 64 or 128) feeding 1x1 / stride 1 / C -> multiple of 128
    if (d1.dtype == GPP_F32) return GPP_ERR_UNSUPPORTED;           // 16-bit storage types, and the x3 types on pre-split maps
    if (is_x3(d1.dtype) && (!(d1.x3_split & GPP_X3_IN) || (d2.x3_split & (GPP_X3_OUT | GPP_X3_RES)) != (GPP_X3_OUT | GPP_X3_RES) || !d2.residual))
        return GPP_ERR_UNSUPPORTED;
    if (d1.dtype != d2.dtype || d1.n_groups != 1 || d2.n_groups != 1 || d1.batch != d2.batch) return GPP_ERR_UNSUPPORTED;
    if (d1.KH != 3 || d1.KW != 3 || d1.stride != 1 || d1.pad_top != 1 || d1.pad_left != 1 || d1.residual || d1.out_f32) return GPP_ERR_UNSUPPORTED;
    if (d1.C_in != d1.C_out || (d1.C_in != 64 && d1.C_in != 128) || d1.weight_rows < d1.C_out) return GPP_ERR_UNSUPPORTED;
    if (d2.KH != 1 || d2.KW != 1 || d2.stride != 1 || d2.pad_top != 0 || d2.pad_left != 0 || d2.C_in != d1.C_out) return GPP_ERR_UNSUPPORTED;
    if (d2.C_out % 128 != 0 || d2.weight_rows < d2.C_out) return GPP_ERR_UNSUPPORTED;
    if (G1.H_in != G1.H_out || G1.W_in != G1.W_out || G2.H_out != G1.H_out || G2.W_out != G1.W_out || G2.H_in != G1.H_out || G2.W_in != G1.W_out)
        return GPP_ERR_BAD_ARG;
    rc = fill_range_counter(d1);
    if (rc == GPP_OK) rc = fill_range_counter(d2);
    if (rc != GPP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    switch (d1.dtype) {
        case GPP_BF16: return gpp_tail_dispatch_bf16(d1, d2, tile_rows, st);
        case GPP_F16: return gpp_tail_dispatch_f16(d1, d2, tile_rows, st);
        case GPP_BF16X3: return gpp_tail_dispatch_bf16x3(d1, d2, tile_rows, st);
        default: return gpp_tail_dispatch_f16x3(d1, d2, tile_rows, st);
    }
}

int block_entry(const gpp_conv_desc* conv_a, const gpp_conv_desc* conv_b, const gpp_conv_desc* conv_c, int tile, void* stream)
{
    if (!conv_a || !conv_b || !conv_c) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d1 = *conv_a, d2 = *conv_b, d3 = *conv_c;
    int rc = validate(d1);
    if (rc == GPP_OK) rc = validate(d2);
    if (rc == GPP_OK) rc = validate(d3);
    if (rc != GPP_OK) return rc;
    if (d1.gather_rows || d2.gather_rows || d3.gather_rows || d1.guard || d2.guard || d3.guard || d1.tower_rows || d2.tower_rows || d3.tower_rows ||
        d1.deep_rows || d2.deep_rows || d3.deep_rows || d1.lists_after || d2.lists_after || d3.lists_after || d1.conv_after || d2.conv_after ||
        d3.conv_after || d1.conv_before || d2.conv_before || d3.conv_before)
        return GPP_ERR_UNSUPPORTED;
    const gpp_conv_group &G1 = d1.groups[0], &G2 = d2.groups[0], &G3 = d3.groups[0];
    // the triple this kernel fuses, on pre-split maps of one x3 type: 1x1 / stride 1 or 2 / C_in -> C; 3x3 / stride 1 / pad 1 / C -> C (C = 64 or 128);
    // 1x1 / stride 1 / C -> a multiple of 128, + shortcut map of the output's size
    if (!is_x3(d1.dtype) || d1.dtype != d2.dtype || d1.dtype != d3.dtype) return GPP_ERR_UNSUPPORTED;
    if (d1.n_groups != 1 || d2.n_groups != 1 || d3.n_groups != 1 || d1.batch != d2.batch || d1.batch != d3.batch) return GPP_ERR_UNSUPPORTED;
    if (d1.x3_split != (GPP_X3_IN | GPP_X3_OUT) || d2.x3_split != (GPP_X3_IN | GPP_X3_OUT) || d3.x3_split != (GPP_X3_IN | GPP_X3_OUT | GPP_X3_RES))
        return GPP_ERR_UNSUPPORTED;
    if (d1.KH != 1 || d1.KW != 1 || d1.pad_top != 0 || d1.pad_left != 0 || d1.residual || d1.out_f32 || d1.split_k > 1) return GPP_ERR_UNSUPPORTED;
    if (d2.KH != 3 || d2.KW != 3 || d2.stride != 1 || d2.pad_top != 1 || d2.pad_left != 1 || d2.residual || d2.out_f32 || d2.split_k > 1) return GPP_ERR_UNSUPPORTED;
    if (d3.KH != 1 || d3.KW != 1 || d3.stride != 1 || d3.pad_top != 0 || d3.pad_left != 0 || !d3.residual || d3.out_f32 || d3.split_k > 1) return GPP_ERR_UNSUPPORTED;
    const int C = d2.C_in;
    if ((C != 64 && C != 128) || d2.C_out != C || d1.C_out != C || d3.C_in != C || d3.C_out % 128 != 0) return GPP_ERR_UNSUPPORTED;
    if (d1.weight_rows < C || d2.weight_rows < C || d3.weight_rows < d3.C_out) return GPP_ERR_UNSUPPORTED;
    if (G1.H_out != (G1.H_in - 1) / d1.stride + 1 || G1.W_out != (G1.W_in - 1) / d1.stride + 1) return GPP_ERR_BAD_ARG;
    if (G2.H_in != G1.H_out || G2.W_in != G1.W_out || G2.H_out != G1.H_out || G2.W_out != G1.W_out || G3.H_in != G1.H_out || G3.W_in != G1.W_out ||
        G3.H_out != G1.H_out || G3.W_out != G1.W_out || G3.H_res != G1.H_out || G3.W_res != G1.W_out)
        return GPP_ERR_BAD_ARG;
    rc = fill_range_counter(d1);
    if (rc == GPP_OK) rc = fill_range_counter(d2);
    if (rc == GPP_OK) rc = fill_range_counter(d3);
    if (rc != GPP_OK) return rc;
    if (d1.range_counter != d3.range_counter || d2.range_counter != d3.range_counter) return GPP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    return d1.dtype == GPP_F16X3 ? gpp_block_dispatch_f16x3(d1, d2, d3, tile, st) : gpp_block_dispatch_bf16x3(d1, d2, d3, tile, st);
}

// the same block with its projection shortcut (conv_p: 1x1 / stride 1 / C_in -> 4 C on the block's own input) computed inside the launch
int block_proj_entry(const gpp_conv_desc* conv_a, const gpp_conv_desc* conv_b, const gpp_conv_desc* conv_c, const gpp_conv_desc* conv_p, int tile,
                     void* stream)
{
    if (!conv_a || !conv_b || !conv_c || !conv_p) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d1 = *conv_a, d2 = *conv_b, d3 = *conv_c, dp = *conv_p;
    int rc = validate(d1);
    if (rc == GPP_OK) rc = validate(d2);
    if (rc == GPP_OK) rc = validate(d3);
    if (rc == GPP_OK) rc = validate(dp);
    if (rc != GPP_OK) return rc;
    for (const gpp_conv_desc* d : {&d1, &d2, &d3, &dp})
        if (d->gather_rows || d->guard || d->tower_rows || d->deep_rows || d->lists_after || d->conv_after || d->conv_before) return GPP_ERR_UNSUPPORTED;
    const gpp_conv_group &G1 = d1.groups[0], &G2 = d2.groups[0], &G3 = d3.groups[0], &GP = dp.groups[0];
    if (!is_x3(d1.dtype) || d1.dtype != d2.dtype || d1.dtype != d3.dtype || d1.dtype != dp.dtype) return GPP_ERR_UNSUPPORTED;
    if (d1.n_groups != 1 || d2.n_groups != 1 || d3.n_groups != 1 || dp.n_groups != 1 || d1.batch != d2.batch || d1.batch != d3.batch || d1.batch != dp.batch)
        return GPP_ERR_UNSUPPORTED;
    // every map between the layers pre-split; the block's input pre-split or float32 (pool1's map), the same for both of its readers
    if ((d1.x3_split | GPP_X3_IN) != (GPP_X3_IN | GPP_X3_OUT) || d2.x3_split != (GPP_X3_IN | GPP_X3_OUT) || d3.x3_split != (GPP_X3_IN | GPP_X3_OUT) ||
        dp.x3_split != d1.x3_split)
        return GPP_ERR_UNSUPPORTED;
    if (d1.KH != 1 || d1.KW != 1 || d1.stride != 1 || d1.pad_top != 0 || d1.pad_left != 0 || d1.residual || d1.out_f32 || d1.split_k > 1) return GPP_ERR_UNSUPPORTED;
    if (d2.KH != 3 || d2.KW != 3 || d2.stride != 1 || d2.pad_top != 1 || d2.pad_left != 1 || d2.residual || d2.out_f32 || d2.split_k > 1) return GPP_ERR_UNSUPPORTED;
    if (d3.KH != 1 || d3.KW != 1 || d3.stride != 1 || d3.pad_top != 0 || d3.pad_left != 0 || d3.residual || d3.out_f32 || d3.split_k > 1) return GPP_ERR_UNSUPPORTED;
    if (dp.KH != 1 || dp.KW != 1 || dp.stride != 1 || dp.pad_top != 0 || dp.pad_left != 0 || dp.residual || dp.relu || dp.out_f32 || dp.split_k > 1) return GPP_ERR_UNSUPPORTED;
    // res2a's shape: 64 -> 64 -> 256 (the kernel's branch1 loop is written for any C_in that is a multiple of 32; only this one is built and tested)
    if (d1.C_in != 64 || d2.C_in != 64 || d2.C_out != 64 || d1.C_out != 64 || d3.C_in != 64 || d3.C_out != 256 || dp.C_out != d3.C_out) return GPP_ERR_UNSUPPORTED;
    if (dp.in != d1.in || dp.in_pitch != d1.in_pitch || dp.C_in != d1.C_in || GP.in_off != G1.in_off || GP.in_bstride != G1.in_bstride ||
        GP.H_in != G1.H_in || GP.W_in != G1.W_in || GP.H_out != G1.H_out || GP.W_out != G1.W_out)
        return GPP_ERR_UNSUPPORTED;
    // (dp.weight_rows >= dp.C_out with dp.C_in == d1.C_in is also what bounds the kernel's plain loads of the branch1 weight fragments)
    if (d1.weight_rows < 64 || d2.weight_rows < 64 || d3.weight_rows < d3.C_out || dp.weight_rows < dp.C_out) return GPP_ERR_UNSUPPORTED;
    if (G1.H_out != G1.H_in || G1.W_out != G1.W_in) return GPP_ERR_BAD_ARG;
    if (G2.H_in != G1.H_out || G2.W_in != G1.W_out || G2.H_out != G1.H_out || G2.W_out != G1.W_out || G3.H_in != G1.H_out || G3.W_in != G1.W_out ||
        G3.H_out != G1.H_out || G3.W_out != G1.W_out)
        return GPP_ERR_BAD_ARG;
    for (gpp_conv_desc* d : {&d1, &d2, &d3, &dp})
        if ((rc = fill_range_counter(*d)) != GPP_OK) return rc;
    if (d1.range_counter != d3.range_counter || d2.range_counter != d3.range_counter || dp.range_counter != d3.range_counter) return GPP_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    return d1.dtype == GPP_F16X3 ? gpp_block_proj_dispatch_f16x3(d1, d2, d3, dp, tile, st) : gpp_block_proj_dispatch_bf16x3(d1, d2, d3, dp, tile, st);
}

// the descriptors gpp_conv_desc.conv_after names by number (gpp_conv2d_deferred_register)
std::mutex g_deferred_mutex;
std::vector<gpp_conv_desc> g_deferred_descs;
std::vector<char> g_deferred_held;

}  // namespace

extern "C" int gpp_bottleneck_block_proj(const gpp_conv_desc* conv1x1_a, const gpp_conv_desc* conv3x3_b, const gpp_conv_desc* conv1x1_c,
                                         const gpp_conv_desc* conv1x1_proj, int tile, void* stream)
{
    return block_proj_entry(conv1x1_a, conv3x3_b, conv1x1_c, conv1x1_proj, tile, stream);
}

extern "C" int gpp_bottleneck_block(const gpp_conv_desc* conv1x1_a, const gpp_conv_desc* conv3x3_b, const gpp_conv_desc* conv1x1_c, int tile, void* stream)
{
    return block_entry(conv1x1_a, conv3x3_b, conv1x1_c, tile, stream);
}

extern "C" int gpp_bottleneck_tail(const gpp_conv_desc* conv3x3, const gpp_conv_desc* conv1x1, int tile_rows, void* stream)
{
    return tail_entry(conv3x3, conv1x1, tile_rows, stream);
}

extern "C" int gpp_x3_range_events(uint64_t* host_count, int reset)
{
    unsigned long long v = 0;
    const int rc = gpp_x3_range_events_f16x3(&v, reset);
    if (rc == GPP_OK && host_count) *host_count = (uint64_t)v;
    return rc;
}

extern "C" int gpp_x3_range_snapshot(uint64_t* device_count, void* stream)
{
    return gpp_x3_range_snapshot_of(nullptr, device_count, stream);
}

extern "C" int gpp_x3_range_snapshot_of(const uint64_t* counter, uint64_t* device_count, void* stream)
{
    if (!device_count) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)counter | (uintptr_t)device_count) & 7) return GPP_ERR_ALIGN;
    return gpp_x3_range_snapshot_f16x3((const unsigned long long*)counter, (unsigned long long*)device_count, (hipStream_t)stream);
}

extern "C" int gpp_conv2d_flops(const gpp_conv_desc* host_desc, double* flops)
{
    if (!host_desc || !flops) return GPP_ERR_BAD_ARG;
    if (host_desc->n_groups < 1 || host_desc->n_groups > GPP_MAX_GROUPS) return GPP_ERR_BAD_ARG;
    double f = 0.0;
    for (int g = 0; g < host_desc->n_groups; ++g)
        f += 2.0 * host_desc->batch * (double)host_desc->groups[g].H_out * host_desc->groups[g].W_out *
             host_desc->KH * host_desc->KW * (double)host_desc->C_in * host_desc->C_out;
    *flops = f;
    return GPP_OK;
}

extern "C" int gpp_conv2d_split_rule(const gpp_conv_desc* host_desc, int* split_k)
{
    if (!host_desc || !split_k) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d = *host_desc;
    int rc = validate(d);
    if (rc != GPP_OK) return rc;
    *split_k = d.split_k > 0 ? d.split_k : split_rule(d);
    return GPP_OK;
}

extern "C" int gpp_conv2d_workspace_bytes(const gpp_conv_desc* host_desc, size_t* bytes)
{
    if (!host_desc || !bytes) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d = *host_desc;
    char probe[16] __attribute__((aligned(16)));
    if (!d.partial) { d.partial = probe; d.partial_bytes = 0; }     // the rule is asked "what if a workspace existed"
    int rc = validate(d);
    if (rc != GPP_OK) return rc;
    const int split = d.split_k > 0 ? d.split_k : split_rule(d);
    *bytes = 0;
    if (split <= 1) return GPP_OK;
    // partial slabs [split][M tiles * BM][N tiles * BN] float32 for the largest block tile (224 rows, 256 columns)
    int64_t rows = 0;
    for (int g = 0; g < d.n_groups; ++g) rows += (int64_t)d.batch * d.groups[g].H_out * d.groups[g].W_out + 256;
    const int64_t npad = (d.C_out + 255) / 256 * 256;
    *bytes = (size_t)(split * rows * npad * 4);
    return GPP_OK;
}

extern "C" int gpp_conv2d_igemm(const gpp_conv_desc* host_desc, void* stream)
{
    if (!host_desc) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d = *host_desc;
    for (int g = 0; g < GPP_MAX_GROUPS; ++g) d.groups[g].row_begin = 0;       // the library's own field (mixed grids)
    int rc = validate(d);
    if (rc != GPP_OK) return rc;
    // lists_after: the deep lists behind this layer's launch on the same stream (the layer writes the logits they are made from); a handle
    // nobody holds is refused before anything is launched
    // conv_after: a layer of both forms behind the lists (their rows are its rows), the same kind of handle
    // conv_before: the registered layer in front, dense -- its lists dropped, its range events into this call's counter -- then this one
    const int32_t lists = d.lists_after, after = d.conv_after, before = d.conv_before;
    d.lists_after = d.conv_after = d.conv_before = 0;
    if (lists && (rc = gpp_detect_deep_lists_run(lists, 1, stream)) != GPP_OK) return rc;
    if (after && (rc = gpp_conv2d_deferred_run(after, 1, stream)) != GPP_OK) return rc;
    if (before) {
        gpp_conv_desc front;
        {
            std::lock_guard<std::mutex> lock(g_deferred_mutex);
            if ((size_t)before > g_deferred_held.size() || !g_deferred_held[(size_t)before - 1]) return GPP_ERR_BAD_ARG;
            front = g_deferred_descs[(size_t)before - 1];
        }
        front.deep_rows = front.deep_counts = front.deep_flag = nullptr;
        front.deep_tile = 0;
        if (d.range_counter) front.range_counter = d.range_counter;
        if ((rc = gpp_conv2d_igemm(&front, stream)) != GPP_OK) return rc;
    }
    rc = dispatch_any(d, (hipStream_t)stream);
    if (rc == GPP_OK && lists) rc = gpp_detect_deep_lists_run(lists, 0, stream);
    if (rc == GPP_OK && after) rc = gpp_conv2d_deferred_run(after, 0, stream);
    return rc;
}

extern "C" int gpp_conv2d_deferred_register(const gpp_conv_desc* host_desc, int32_t* handle)
{
    if (!host_desc || !handle) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d = *host_desc;
    for (int g = 0; g < GPP_MAX_GROUPS; ++g) d.groups[g].row_begin = 0;
    const int rc = validate(d);
    if (rc != GPP_OK) return rc;
    // a layer of both forms on the deep lists, and the end of the chain: what it names cannot name another
    if (!d.deep_rows || d.lists_after || d.conv_after || d.conv_before) return GPP_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(g_deferred_mutex);
    size_t slot = 0;
    while (slot < g_deferred_held.size() && g_deferred_held[slot]) ++slot;
    if (slot >= (size_t)INT_MAX - 1) return GPP_ERR_UNSUPPORTED;
    if (slot == g_deferred_held.size()) { g_deferred_held.push_back(0); g_deferred_descs.push_back(d); }
    g_deferred_descs[slot] = d;
    g_deferred_held[slot] = 1;
    *handle = (int32_t)slot + 1;
    return GPP_OK;
}

extern "C" int gpp_conv2d_deferred_release(int32_t handle)
{
    std::lock_guard<std::mutex> lock(g_deferred_mutex);
    if (handle < 1 || (size_t)handle > g_deferred_held.size() || !g_deferred_held[(size_t)handle - 1]) return GPP_ERR_BAD_ARG;
    g_deferred_held[(size_t)handle - 1] = 0;
    return GPP_OK;
}

extern "C" int gpp_conv2d_deferred_run(int32_t handle, int check_only, void* stream)
{
    gpp_conv_desc d;
    {
        std::lock_guard<std::mutex> lock(g_deferred_mutex);
        if (handle < 1 || (size_t)handle > g_deferred_held.size() || !g_deferred_held[(size_t)handle - 1]) return GPP_ERR_BAD_ARG;
        d = g_deferred_descs[(size_t)handle - 1];
    }
    return check_only ? GPP_OK : gpp_conv2d_igemm(&d, stream);
}

// The block tiles a layer may run with (same K order per output element in every one of them: the choice never changes a result): the
// catalogue's candidates (conv_tiles.h) behind 0 = the library's heuristic.  One list for the autotuner below and for
// gpp_conv2d_tile_candidates (tests draw tiles at random from it).
static const gpp_tiles::Entry kTiles[] = {{0, gpp_tiles::PLAIN, gpp_tiles::ALL, 0, 128, 0, 0, 0}, GPP_CONV_TILES(GPP_TILE_ENTRY, GPP_TILE_NONE, GPP_TILE_NONE)};

static bool env_is_1(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }

static bool tile_is_candidate(const gpp_conv_desc* desc, const gpp_tiles::Entry& t)
{
    using namespace gpp_tiles;
    const gpp_conv_desc& d = *desc;
    // gathered rows: their own tiles (the plain ones for a float32 output, the pipelined ones for a pre-split one), and nobody else's
    const int gform = !d.gather_rows ? -1 : (d.out_f32 ? (int)GATHER : (int)GATHER_PIPE);
    if ((gform >= 0 || t.form == GATHER || t.form == GATHER_PIPE) && t.form != gform) return t.code == 0 && gform >= 0;
    // ---- cannot run: nobody's instantiation, or the form's hard conditions (the dispatcher and the launchers refuse on the same functions)
    const bool x3_in = is_x3(d.dtype) && (d.x3_split & GPP_X3_IN);
    if (!owner_has(t.owner, f32_storage(d.dtype), is_x3(d.dtype))) return false;
    // (pinned, tests/test_tile_table_cpu.py: 192160 stays listed for an x3 layer on a float32 input map, where dispatch refuses it)
    if (is_x3(d.dtype) && x3_wants_split_input(t.form, t.owner) && !x3_in && t.owner != ALL_X3IN) return false;
    const int nk = d.KH * d.KW * (d.C_in / (128 / elem_size(d.dtype)));
    if (t.form == DUAL && !dual_can_run(d, nk)) return false;
    if (t.form == MIX && !mix_can_run(d, nk)) return false;
    if (t.form == WS && !ws_can_run(d, t.bm, t.bn)) return false;
    // ---- not worth timing: tuning heuristics, and the A/B switches GPP_NO_{DEEP,WS,MIX}_TILES=1
    static const bool no_deep = env_is_1("GPP_NO_DEEP_TILES"), no_ws = env_is_1("GPP_NO_WS_TILES"), no_mix = env_is_1("GPP_NO_MIX_TILES");
    int64_t rows = 0;
    for (int g = 0; g < d.n_groups; ++g) rows += (int64_t)d.batch * d.groups[g].H_out * d.groups[g].W_out;
    const int bn = t.bn;
    const auto pads_less_than = [&](int other) { return (d.C_out + bn - 1) / bn * bn < (d.C_out + other - 1) / other * other; };
    switch (t.form) {
        case GATHER: return bn != 160 || pads_less_than(64);                // 160 columns only where that cuts the N padding
        case GATHER_PIPE: return gather_pipe_can_run(d);
        case DEEP: {                                                         // deep K, and a grid of at most ~one workgroup per CU
            int64_t tiles_m = 0;
            for (int g = 0; g < d.n_groups; ++g) tiles_m += ((int64_t)d.batch * d.groups[g].H_out * d.groups[g].W_out + t.bm - 1) / t.bm;
            const int64_t wgs = tiles_m * ((d.C_out + bn - 1) / bn) * (d.split_k > 1 ? d.split_k : 1);
            return !(bn == 64 && d.C_out > 256) && !no_deep && nk >= 12 && wgs <= 320;
        }
        case WS: return !no_ws && rows >= 256 * 16;
        case MIX: return !no_mix && nk >= 4 && rows * (d.C_out / 256) >= 256 * 256;      // enough rows for two rounds
        default: break;
    }
    if (t.code == 0) return true;
    // narrow tiles on wide layers: never competitive -- except on the shallow 1 x 1 layers (K <= 256: a handful of K-steps, bound by the
    // latency of their few dependent tile loads, where more and smaller workgroups per CU win 3 - 6 %: profiles/r4/hbm_layers_f16x3.txt)
    if (bn == 64 && d.C_out > 256 && !(d.KH == 1 && d.KW == 1 && d.C_in <= 256)) return false;
    if (bn == 256 && (d.C_out < 192 || rows < 256 * 16)) return false;
    if ((t.form == PIPE || t.form == DUAL) && nk < 4) return false;          // the pipelined loops need a few K-steps to pay
    if ((bn == 160 || bn == 96) && !pads_less_than(128)) return false;      // only where it cuts the N padding (144 regression channels, 96 logits)
    return true;
}

extern "C" int gpp_conv2d_tile_candidates(const gpp_conv_desc* desc, int* tiles, int capacity, int* count)
{
    if (!desc || !count || capacity < 0 || (capacity > 0 && !tiles)) return GPP_ERR_BAD_ARG;
    {
        gpp_conv_desc d = *desc;
        for (int g = 0; g < GPP_MAX_GROUPS; ++g) d.groups[g].row_begin = 0;
        const int rc = validate(d);
        if (rc != GPP_OK) return rc;
    }
    int n = 0;
    for (const gpp_tiles::Entry& t : kTiles) {
        if (!tile_is_candidate(desc, t)) continue;
        if (n < capacity) tiles[n] = t.code;
        ++n;
    }
    *count = n;
    return GPP_OK;
}

// Pick the fastest block tile for one layer by timing the candidates on the device (the layer is idempotent: it only
// rewrites its own output).  The tile-count arithmetic (how many workgroups land on 256 CUs, in how many rounds) decides
// most mid-sized layers and is not worth modelling: measure.  Writes the winner into desc->tile_hint.  The tile never
// changes a result (same K order per output element); split-K would, and is therefore NOT tuned: desc->split_k is used as
// given (0 = gpp_conv2d_split_rule).
extern "C" int gpp_conv2d_autotune(gpp_conv_desc* desc, int iters, void* stream, float* best_us)
{
    if (!desc || iters < 1) return GPP_ERR_BAD_ARG;
    {
        gpp_conv_desc d = *desc;
        for (int g = 0; g < GPP_MAX_GROUPS; ++g) d.groups[g].row_begin = 0;
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
    const int32_t lists_in = desc->lists_after, after_in = desc->conv_after, before_in = desc->conv_before;
    desc->lists_after = desc->conv_after = desc->conv_before = 0;                        // the layer's own launch is what is timed, not the lists or the layer behind it
    float best = 1e30f;
    int best_tile = tile_in, rc = GPP_OK;
    auto time_one = [&](int tile, float* us, int reps = 2) -> int {
        desc->tile_hint = tile;
        int r = gpp_conv2d_igemm(desc, stream);                      // warm-up (and validity of this choice)
        if (r != GPP_OK) return r;
        float t_best = 1e30f;
        for (int rep = 0; rep < reps; ++rep) {
            (void)hipEventRecord(e0, st);
            for (int i = 0; i < iters; ++i) (void)gpp_conv2d_igemm(desc, stream);
            (void)hipEventRecord(e1, st);
            hipError_t s = hipEventSynchronize(e1);
            if (s != hipSuccess) return (int)s;
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            t_best = ms < t_best ? ms : t_best;
        }
        *us = t_best * 1000.0f / iters;
        return GPP_OK;
    };
    float second = 1e30f;
    int second_tile = -1;
    for (const gpp_tiles::Entry& t : kTiles) {
        if (!tile_is_candidate(desc, t)) continue;
        const int tile = t.code;
        float us = 0.0f;
        int r = time_one(tile, &us);
        if (r != GPP_OK) { if (tile == 0) { rc = r; break; } continue; }
        if (us < best) { second = best; second_tile = best_tile; best = us; best_tile = tile; }
        else if (us < second) { second = us; second_tile = tile; }
    }
    // A play-off when the two fastest are within 5 %: the sweep times its candidates one after the other while the board's clock settles under the
    // load (a power-bound layer runs 2 - 4 % faster in the first tenths of a second), so its order can decide a close call -- round 6 saw one of the
    // three identical regression-tower layers take the uniform 256 x 256 grid (841 us) beside two that took the mixed-height one (806 - 820).
    // Three alternating rounds, the sum decides.
    if (rc == GPP_OK && second_tile >= 0 && second_tile != best_tile && second <= best * 1.05f) {
        float sum_a = 0.0f, sum_b = 0.0f;
        bool ok = true;
        for (int round = 0; round < 3 && ok; ++round) {
            float a = 0.0f, b = 0.0f;
            ok = time_one(best_tile, &a, 1) == GPP_OK && time_one(second_tile, &b, 1) == GPP_OK;
            sum_a += a;
            sum_b += b;
        }
        if (ok && sum_b < sum_a) { best_tile = second_tile; best = sum_b / 3.0f; }
        else if (ok) best = sum_a / 3.0f;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    desc->tile_hint = rc == GPP_OK ? best_tile : tile_in;
    desc->lists_after = lists_in;
    desc->conv_after = after_in;
    desc->conv_before = before_in;
    if (best_us) *best_us = best;
    return rc;
}

// ---- gpp_conv2d_preact: the 1 x 1 convolution of a DenseNet layer with its input's BatchNormalization + ReLU as a prologue
// (conv_igemm_impl.h: PRE).  Scope: 1 x 1, stride 1, pad 0 (a padded zero would become relu(shift)), float32-sized input map that is
// not pre-split, GPP_F32 / GPP_F16X3 / GPP_BF16X3.
namespace {

#define GPP_TILE_CODE(code, ...) code,
static const int kPreactTiles[] = {0, GPP_CONV_TILES(GPP_TILE_NONE, GPP_TILE_NONE, GPP_TILE_CODE)};
#undef GPP_TILE_CODE

int preact_validate(gpp_conv_desc& d, const float* in_scale, const float* in_shift)
{
    for (int g = 0; g < GPP_MAX_GROUPS; ++g) d.groups[g].row_begin = 0;
    int rc = validate(d);
    if (rc != GPP_OK) return rc;
    if (d.dtype != GPP_F32 && !is_x3(d.dtype)) return GPP_ERR_UNSUPPORTED;
    if (!in_scale || !in_shift) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)in_scale | (uintptr_t)in_shift) & 15) return GPP_ERR_ALIGN;
    if (d.KH != 1 || d.KW != 1 || d.stride != 1 || d.pad_top != 0 || d.pad_left != 0) return GPP_ERR_UNSUPPORTED;
    if (d.x3_split & GPP_X3_IN) return GPP_ERR_UNSUPPORTED;
    if (d.gather_rows || d.guard || d.tower_rows || d.deep_rows || d.lists_after || d.conv_after || d.conv_before) return GPP_ERR_UNSUPPORTED;          // gpp_conv2d_igemm only
    if (d.C_in > 4096) return GPP_ERR_UNSUPPORTED;               // the scale / shift table lives in LDS beside the ring
    return GPP_OK;
}

int preact_run(gpp_conv_desc& d, const float* in_scale, const float* in_shift, hipStream_t st)
{
    int rc = fill_range_counter(d);
    if (rc != GPP_OK) return rc;
    if (d.split_k == 0) d.split_k = split_rule(d);
    switch (d.dtype) {
        case GPP_BF16X3: return gpp_preact_dispatch_bf16x3(d, in_scale, in_shift, st);
        case GPP_F16X3: return gpp_preact_dispatch_f16x3(d, in_scale, in_shift, st);
        default: return gpp_preact_dispatch_f32(d, in_scale, in_shift, st);
    }
}

}  // namespace

extern "C" int gpp_conv2d_preact(const gpp_conv_desc* host_desc, const float* in_scale, const float* in_shift, void* stream)
{
    if (!host_desc) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d = *host_desc;
    const int rc = preact_validate(d, in_scale, in_shift);
    if (rc != GPP_OK) return rc;
    return preact_run(d, in_scale, in_shift, (hipStream_t)stream);
}

extern "C" int gpp_conv2d_preact_tile_candidates(const gpp_conv_desc* desc, int* tiles, int capacity, int* count)
{
    if (!desc || !count || capacity < 0 || (capacity > 0 && !tiles)) return GPP_ERR_BAD_ARG;
    gpp_conv_desc d = *desc;
    static const float probe[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};     // (the tables are not read here)
    const int rc = preact_validate(d, probe, probe);
    if (rc != GPP_OK) return rc;
    int n = 0;
    for (int tile : kPreactTiles) {
        if (n < capacity) tiles[n] = tile;
        ++n;
    }
    *count = n;
    return GPP_OK;
}

extern "C" int gpp_conv2d_preact_autotune(gpp_conv_desc* desc, const float* in_scale, const float* in_shift, int iters, void* stream,
                                          float* best_us)
{
    if (!desc || iters < 1) return GPP_ERR_BAD_ARG;
    {
        gpp_conv_desc d = *desc;
        const int rc = preact_validate(d, in_scale, in_shift);
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
    for (int tile : kPreactTiles) {
        desc->tile_hint = tile;
        int r = gpp_conv2d_preact(desc, in_scale, in_shift, stream);      // warm-up (and validity of this choice)
        if (r != GPP_OK) { if (tile == 0) { rc = r; break; } continue; }
        float t_best = 1e30f;
        for (int rep = 0; rep < 2 && r == GPP_OK; ++rep) {
            (void)hipEventRecord(e0, st);
            for (int i = 0; i < iters; ++i) (void)gpp_conv2d_preact(desc, in_scale, in_shift, stream);
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
