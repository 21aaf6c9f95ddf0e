/*
 * gpp.h -- C ABI of libgpp_hip.so: the MI355X (gfx950) implementation of the data-parallel
 * hot path of arangesh/Ground-Plane-Polling, i.e. everything that one
 *     model.predict_on_batch([images, P_inv, planes])
 * (reference keras_retinanet_3D/bin/run_network.py:110) executes on the device:
 * RetinaNet-3D forward (ResNet + FPN + three heads), anchor decode, NMS / top-k, and the
 * per-detection ground-plane polling.
 *
 * The reference has no native code and no FFI; its "operator API" for this path is the
 * alias table keras_retinanet_3D/backend/tensorflow_backend.py:20-156 plus the Keras layers
 * in keras_retinanet_3D/layers/.  Each entry point below names the reference code it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns int: 0 = GPP_OK, < 0 = argument error (below), > 0 = hipError_t
 *   - never throws, never aborts, allocates nothing: the caller owns every buffer, including
 *     workspaces whose sizes are reported by the *_workspace_bytes functions
 *   - all pointers are DEVICE pointers unless named host_*; kernels are enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream) and run asynchronously
 *   - no global state except per-device launch configuration and the side streams of gpp_plan_run lanes (both
 *     created on first use under a lock, one set per device); safe to call from several host threads on distinct streams
 *   - tensors are dense, row-major, NHWC for images / feature maps
 */
#ifndef GPP_H_
#define GPP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPP_OK 0
#define GPP_ERR_BAD_ARG (-1)    /* null pointer, negative size, unsupported shape */
#define GPP_ERR_WORKSPACE (-2)  /* workspace too small */
#define GPP_ERR_ALIGN (-3)      /* pointer not aligned as documented */
#define GPP_ERR_UNSUPPORTED (-4)

/* Library / build identification: "gpp-hip <version> gfx950". Host pointer, static storage. */
const char* gpp_version(void);

/* ------------------------------------------------------------------------------------------
 * Ground-plane polling.
 * Replaces layers/fit_road_planes.py:49-139 `fit_road_planes` (+ `poll` :18-32, `calc_X_t`
 * :34-47) and the `FitRoadPlanes` layer :142-186.
 *
 *   boxes      (B, D, 12) f32   x1 y1 x2 y2 xl yl xm ym xr yr xt yt   (-1 rows = padding)
 *   dims       (B, D, 3)  f32   h w l
 *   orient     (B, D)     i32   orientation class 0..3, -1 = padding
 *   P_inv      (B, 4, 3)  f32   pseudo-inverse of the scaled camera matrix
 *   planes     (N, 4) f32 if planes_batched == 0 (one database shared by the batch), else
 *              (B, N, 4) as the reference feeds it (preprocessing/kitti.py:220); 16-byte aligned
 *   thr        poll threshold in metres (reference constant 0.7, fit_road_planes.py:94)
 *   keypoints  (B, D, 4, 3) f32  X_l X_m X_r X_t on the selected plane
 *   keyplanes  (B, D, 1, 4) f32  the selected plane, canonicalised (normal up, unit norm)
 *   residuals  (B, D)     f32   masked residual of the selected plane / 6
 *   best_idx   (B, D)     i32   index of the selected plane (may be NULL; the reference
 *                               computes it at :119 but never returns it)
 *   workspace  gpp_poll_workspace_bytes() bytes, 16-byte aligned (canonical planes)
 * ---------------------------------------------------------------------------------------- */
int gpp_poll_workspace_bytes(int B, int N, int planes_batched, size_t* bytes);

int gpp_poll_f32(const float* boxes, const float* dims, const int32_t* orient, const float* P_inv,
                 const float* planes, int B, int D, int N, int planes_batched, float thr,
                 float* keypoints, float* keyplanes, float* residuals, int32_t* best_idx,
                 void* workspace, size_t workspace_bytes, void* stream);


/* ------------------------------------------------------------------------------------------
 * Element types of activations / weights of the convolution kernels.
 * ---------------------------------------------------------------------------------------- */
#define GPP_BF16 1   /* bfloat16 storage, float32 MFMA accumulation (default compute type) */
#define GPP_F16 2    /* IEEE half storage, float32 MFMA accumulation */
#define GPP_F32 3    /* float32 storage AND float32 operands (v_mfma_f32_16x16x4_f32: every product rounded once, float32
                        accumulation): the arithmetic type of the reference, keras.backend.floatx() = float32
                        (utils/image.py:47, placeholders models/retinanet.py:395-396).  1/16 of the 16-bit MFMA rate. */
#define GPP_BF16X3 4 /* float32 storage, each float32 product as three bf16 matrix products: x = hi + lo (hi = bf16(x), lo =
                        bf16(x - hi)), x*w ~ hi*whi + hi*wlo + lo*whi, float32 accumulation: ~2^-16 relative error per product
                        (float32: 2^-24, plain bf16 operands: 2^-8) at a third of the bf16 MFMA rate.  Activations, residuals
                        and outputs are float32 exactly as for GPP_F32; the weight matrix holds, per K-step of 32 input
                        channels, the 32 bf16 hi parts followed by the 32 bf16 lo parts (same bytes per row as float32). */
#define GPP_F16X3 5  /* as GPP_BF16X3 with IEEE-half halves: hi = f16(x), lo = f16(x - hi), 11 + 11 significant bits, ~2^-22 relative
                        error per product (float32: 2^-24): the throughput mode that stays inside the reference-precision tolerance
                        (plane index exact, 3-D corners within 1e-3 of the float32 path).  Range: finite activations beyond +-65504 are
                        clamped when they are split and COUNTED (gpp_x3_range_events below); a non-finite activation stays non-finite
                        (hi = x, lo = x - x: NaN or inf), as in the float32 path -- a broken activation is never laundered into a
                        plausible finite value; the packed weights of an output channel are scaled by a power of two so that
                        both halves are normal halfs, and gpp_conv_desc.out_scale (float32 per output channel, the inverse power of
                        two) is applied to the accumulator before the bias. */

/* ------------------------------------------------------------------------------------------
 * 2-D convolution, NHWC, implicit GEMM on MFMA (no im2col buffer), fused epilogue
 *     out = act( conv(in, weight) + bias [+ nearest_resize(residual)] )
 * Replaces every Conv2D (+ frozen BatchNormalization folded into weight/bias, + ReLU, + Add,
 * + UpsampleLike) of the graph built by models/retinanet.py:24-205 (heads :24-167, FPN
 * :170-205; UpsampleLike layers/_misc.py:90-100) and of the third-party keras_resnet
 * bottleneck stack instantiated at models/resnet.py:88-93, except the 3-channel stem.
 *
 * One launch covers up to GPP_MAX_GROUPS independent feature maps that share the weights
 * (the five pyramid levels of a head layer, retinanet.py:257-281), each described by a
 * gpp_conv_group.  GEMM view per group: M = batch*H_out*W_out output pixels, N = C_out,
 * K = KH*KW*C_in, K ordered (c_in / CK, kh, kw, c_in % CK) with CK = 128 bytes of channels (64 for the 16-bit types,
 * 32 for the float32-sized types GPP_F32 / GPP_BF16X3 / GPP_F16X3): the taps of one channel chunk are adjacent so that their
 * overlapping input rows are re-read from the XCD-local L2.
 *
 * Layouts (element = 2 bytes for GPP_BF16 / GPP_F16, 4 bytes for GPP_F32 / GPP_BF16X3 / GPP_F16X3; a pre-split x3 map, see x3_split,
 * has the same 4 bytes per element: 32 channels = 64 bytes of hi halves + 64 bytes of lo halves)
 *   in        pixel (b, y, x) of a group at  in + in_off + b*in_bstride + (y*W_in + x)*in_pitch,
 *             C_in contiguous channels there (in_pitch >= C_in lets a channel slice be read)
 *   weight    [C_out rounded up to a multiple of 256][KH*KW*C_in], K contiguous; rows >= C_out
 *             must exist (zero) -- weight_rows states how many rows are allocated.  Rows are
 *             interleaved within every group of 32 output channels: stored row 16h + 4q + r holds
 *             output channel 8q + 4h + r (h in 0..1, q, r in 0..3), so that a lane of the MFMA result
 *             owns 8 consecutive output channels (16-byte stores straight from the accumulators)
 *   bias      [C_out] float32 (NULL = none)
 *   residual  same addressing as out with res_* fields; when H_res/W_res differ from
 *             H_out/W_out the residual is read with TF nearest-neighbour resize semantics
 *             src = min(floor(dst * in/out), in-1)  (tf.image.resize_images, align_corners=False)
 *   out       element type = dtype, or float32 when out_f32 != 0
 *   zero_page unused since v0.2 (padding comes from range-checked buffer loads); may be NULL
 * Requirements: C_in % CK == 0; C_out % 4 == 0; in_pitch, out_pitch, res_pitch multiples of 16 bytes
 * (8 elements; 4 for float32); all base pointers 16-byte aligned; stride in {1, 2}.
 * Padding is explicit (pad_top, pad_left); bottom/right padding is implied by H_out/W_out
 * (this covers Keras 'same' at stride 1, TF's asymmetric 'same' at stride 2, and
 * ZeroPadding2D + 'valid').  Every input map and the weight tensor must be smaller than 2 GiB.
 * Supported and tested geometry: KH, KW each in 1..8 (square or not, odd or even; 9 and up is GPP_ERR_UNSUPPORTED), any
 * pad_top / pad_left >= 0 -- beyond K/2 and beyond the map's size included -- stride 1 or 2, any H_out / W_out >= 1: an output
 * pixel none of whose taps lands on the map is act(bias).  Every tile code an element type owns computes every such layer with the
 * bits of the default tile or refuses it for its own documented reason (tests/test_conv_geometry_gpu.py, ..._cpu.py: kernels from
 * 1x7 / 7x1 to 8x8 against a float64 convolution, split-K, the dual / mixed grids and the gathered forms included).  Negative pads
 * and strides above 2 are not supported.
 * ---------------------------------------------------------------------------------------- */
#define GPP_MAX_GROUPS 5

typedef struct gpp_conv_group {
    int64_t in_off, in_bstride;     /* elements */
    int64_t out_off, out_bstride;
    int64_t res_off, res_bstride;
    int32_t H_in, W_in, H_out, W_out;
    int32_t H_res, W_res;
    int32_t tile_start;             /* filled in by the library */
    int32_t row_begin;              /* filled in by the library (first GEMM row of the group this grid part covers; callers leave 0) */
} gpp_conv_group;

typedef struct gpp_conv_desc {
    const void* in;
    const void* weight;
    const float* bias;
    const void* residual;
    void* out;
    const void* zero_page;
    int32_t dtype;                  /* GPP_BF16 | GPP_F16 | GPP_F32 | GPP_BF16X3 | GPP_F16X3 */
    int32_t out_f32;
    int32_t batch, C_in, C_out, KH, KW, stride, pad_top, pad_left;
    int32_t in_pitch, out_pitch, res_pitch;   /* elements per pixel */
    int32_t weight_rows;
    int32_t relu;
    int32_t n_groups;
    int32_t tile_hint;              /* 0 = library heuristic; otherwise a block tile, by family:
                                         BM * 1000 + BN          the plain loop (legacy aliases 64 / 128 / 256 / 512)
                                         1000000 + BM * 1000 + BN   the software-pipelined loop
                                         2256256                 256 x 256 tiles + 512 x 128 tiles for the last 128 columns, one grid
                                         3000000 + BMA * 1000 + BMB  256-column tiles of two heights in one grid
                                         4000000 + BM * 1000 + BN   the weight-stationary persistent 1 x 1
                                         5000000 + BM * 1000 + BN   the plain loop on a four-deep LDS ring
                                         6000000 / 7000000 + BM * 1000 + BN   gathered rows (gather_rows), two- / four-deep ring
                                         8000000 + BM * 1000 + 256  gathered rows into a pre-split map, the pipelined loop (BM 0: chosen on the device)
                                       A code nobody has: GPP_ERR_BAD_ARG; one this element type, input form or layer cannot run:
                                       GPP_ERR_UNSUPPORTED.  The catalogue is csrc/conv_tiles.h; gpp_conv2d_tile_candidates lists
                                       what a layer accepts; see gpp_conv2d_autotune */
    int32_t reserved;               /* must be 0 (anything else: GPP_ERR_BAD_ARG).  Only the diagnostic -DGPP_STAMPS build of the
                                       library (make stamps; tools/bench_conv.py) reads it: bit 0 skip the tile loads, bit 1 skip
                                       the LDS reads + MFMA, bit 2 / 3 flip the pipelined form of the 128128 / 256256 tile,
                                       bits 4, 5 enable in-kernel time stamps (written through zero_page) */
    int32_t in_bytes, weight_bytes; /* filled in by the library: extents for the range-checked buffer loads */
    void* partial;                  /* optional split-K workspace (float32 partial tiles), 16-byte aligned; NULL = never split */
    int64_t partial_bytes;          /* >= gpp_conv2d_workspace_bytes(), else GPP_ERR_WORKSPACE when the layer is split */
    int32_t split_k;                /* 0 = gpp_conv2d_split_rule (a function of the layer alone), 1 = never, k > 1 = exactly k */
    int32_t partial_rows;           /* filled in by the library */
    gpp_conv_group groups[GPP_MAX_GROUPS];
    int32_t x3_split;               /* GPP_BF16X3 / GPP_F16X3 only (0 otherwise): which of the float32-sized maps hold PRE-SPLIT values, bits
                                       GPP_X3_IN | GPP_X3_OUT | GPP_X3_RES.  A pre-split map stores every 32 channels of a pixel
                                       (128 bytes) as [32 bf16 hi | 32 bf16 lo], hi = bf16(x), lo = bf16(x - hi) -- the layout the
                                       packed weights already have -- instead of 32 float32: the matrix loop then takes its
                                       operands straight from LDS, without the per-fragment split on the vector ALU that shares
                                       issue slots with the matrix pipe.  Needs pitches and offsets that are multiples of 32
                                       channels; an output map can be pre-split only when out_f32 == 0 and C_out % 32 == 0 */
    int32_t reserved2;              /* must be 0 */
    const float* out_scale;         /* GPP_F16X3 only (NULL otherwise, and NULL = all ones): per output channel, accumulator *= out_scale[n]
                                       before the bias -- the inverse of the power of two the channel's packed weights were scaled by */
    uint64_t* range_counter;        /* GPP_F16X3 only: device address of the 8-byte counter this launch adds its range events to (see
                                       gpp_x3_range_events below) -- a caller that runs several models or streams gives each plan a slot of
                                       its own and reads THAT (gpp_x3_range_snapshot_of); NULL = the library's per-device counter */
    const int32_t* gather_rows;     /* NULL = the dense launch.  Otherwise the GATHERED-ROW form: GEMM row m of group g is not pixel m but pixel
                                       list_g[m], and only gather_counts[g] rows exist.  list_g = gather_rows + batch * (pixels of the groups before g):
                                       device int32, the pixel indices b * H_out * W_out + p of that group in ascending order, each at most once.
                                       Every listed pixel receives exactly the bytes the dense launch stores there (same K order, same epilogue);
                                       no other byte of the output map is written.  The grid is sized for every pixel; a workgroup whose first row
                                       lies at or past the count returns at once.  Scope: stride 1, no residual, no split-K (split_k 0 or 1 and a
                                       layer the split rule does not split: GPP_ERR_UNSUPPORTED otherwise), out_f32 output; every dtype.
                                       tile_hint: 0, 6064064, 6032064, 6064160 (6000000 + BM * 1000 + BN: two-deep ring) or 7064064, 7032064,
                                       7064160 (four-deep ring), all with the same bytes */
    const int32_t* gather_counts;   /* device int32 [n_groups] (values outside [0, batch * H_out * W_out] are clamped into it) */
    const int32_t* guard;           /* NULL = none.  Otherwise a device int32 every workgroup reads first: the launch does its work only while
                                       *guard == guard_value and returns at once otherwise -- a launch that a value computed earlier on the
                                       device switches off, without a host round trip.  gpp_conv2d_igemm only (dense or gathered; not the
                                       weight-stationary tiles 4xxxxxx) */
    int32_t guard_value;
    int32_t reserved3;              /* must be 0 */
    const int32_t* tower_rows;      /* NULL = none (then tower_counts and tower_flag are NULL too).  Otherwise ONE call runs BOTH forms of the layer
                                       on the stream, and a device word selects which of them does the work: the dense launch (tile_hint) while
                                       *tower_flag == 1, the gathered-row launch on tower_rows / tower_counts (laid out as gather_rows /
                                       gather_counts; tile tower_tile) while *tower_flag == 0; the workgroups of the other one return on their
                                       first load.  For a layer whose only reader takes it at listed pixels (the last layer of the regression
                                       tower, read by the gathered output layer at the candidates' 3 x 3 neighbourhoods).  gather_rows and
                                       guard stay NULL.  Scope: the gathered form with a pre-split output map, below */
    const int32_t* tower_counts;
    const int32_t* tower_flag;
    int32_t tower_tile;             /* tile of the gathered launch of such a pair: 0 or an 8xxxxxx code */
    int32_t reserved4;              /* must be 0 */
    const int32_t* deep_rows;       /* NULL = none.  Otherwise what tower_rows / tower_counts / tower_flag / tower_tile are, for a tower layer further up
                                       (layers 1 and 2 of the regression tower, on the 7 x 7 and the 5 x 5 neighbourhoods of the candidates' pixels):
                                       both forms behind one call, *deep_flag == 1 the dense launch works, == 0 the gathered one on deep_rows /
                                       deep_counts with tile deep_tile.  Same scope, same checks; the lists are those of gpp_detect_deep_lists, written
                                       on the caller's stream.  All three or none; not together with tower_rows, gather_rows or guard */
    const int32_t* deep_counts;
    const int32_t* deep_flag;
    int32_t deep_tile;              /* 0 or an 8xxxxxx code */
    int32_t lists_after;            /* 0 = none.  Otherwise a handle of gpp_detect_deep_lists_register: gpp_conv2d_igemm enqueues gpp_detect_deep_lists
                                       of that descriptor behind the layer's own launch, on the same stream (the layer that writes the logits).  A
                                       handle nobody holds: GPP_ERR_BAD_ARG, nothing launched.  gpp_conv2d_igemm only */
    int32_t conv_after;             /* 0 = none.  Otherwise a handle of gpp_conv2d_deferred_register: gpp_conv2d_igemm enqueues that descriptor -- a layer
                                       of both forms on deep_rows / deep_counts / deep_flag -- behind this layer's launch AND behind the lists of
                                       lists_after, on the same stream: the regression slice of the towers' fused first layer, whose rows
                                       (gpp_deep_list_desc.rows0) only exist once the logits do.  A handle nobody holds: GPP_ERR_BAD_ARG, nothing
                                       launched.  Not together with gather_rows, guard, tower_rows or deep_rows of this descriptor.
                                       gpp_conv2d_igemm only */
    int32_t conv_before;            /* 0 = none.  Otherwise a handle of gpp_conv2d_deferred_register on a PLAIN dense call of the layer that reads that
                                       layer's map (no lists or guard of its own: GPP_ERR_BAD_ARG otherwise): gpp_conv2d_igemm first enqueues the
                                       registered layer DENSE -- without its lists, its range events into THIS call's range_counter -- and then
                                       this layer.  A dense reader reads every row of the layer in front of it: whoever completes a map that a
                                       run wrote on listed rows only names the layer in front this way, and the library runs the copy it holds.
                                       A handle nobody holds: GPP_ERR_BAD_ARG, nothing launched.  gpp_conv2d_igemm only */
} gpp_conv_desc;
/* The gathered-row form of a layer between two convolutions (gather_rows set, out_f32 == 0): GPP_BF16X3 / GPP_F16X3 with pre-split input AND
 * output maps (x3_split & (GPP_X3_IN | GPP_X3_OUT) both set), stride 1, no shortcut, never split-K, C_out a multiple of 256; anything else
 * with out_f32 == 0 answers GPP_ERR_UNSUPPORTED, as it always has.  It runs the three-phase pipelined loop on 256-column tiles:
 *   tile_hint 8128256, 8160256, 8192256, 8224256, 8256256   tiles of that many rows
 *             0 or 8000256                                    the height is chosen ON THE DEVICE from the counts: the one whose grid costs the
 *                                                             fewest rounds x rows on the chip's 256 compute units (the host cannot know the count)
 * Row tiles are numbered over the LISTED rows (the live workgroups are the first of the grid); every listed row receives the bytes of the
 * dense launch in both halves of the split map, no other byte is written, and GPP_F16X3 range events are counted on the listed rows only. */
#define GPP_X3_IN 1
#define GPP_X3_OUT 2
#define GPP_X3_RES 4

int gpp_conv2d_igemm(const gpp_conv_desc* host_desc, void* stream);
/* gpp_conv_desc.conv_after: the library keeps a copy of a descriptor -- validated as gpp_conv2d_igemm validates it, a layer of both forms on
 * deep_rows / deep_counts / deep_flag, itself without lists_after / conv_after: GPP_ERR_BAD_ARG otherwise -- and hands out a handle > 0 (a
 * number, not an address, as gpp_detect_deep_lists_register does).  gpp_conv2d_deferred_run: gpp_conv2d_igemm of the copy (check_only != 0:
 * whether somebody holds the handle, nothing launched). */
int gpp_conv2d_deferred_register(const gpp_conv_desc* host_desc, int32_t* handle);
int gpp_conv2d_deferred_release(int32_t handle);
int gpp_conv2d_deferred_run(int32_t handle, int check_only, void* stream);

/* Split-K factor the library uses for this layer when desc->split_k == 0 and a workspace is given.  It is a function of
   the layer alone (kernel size, channels, output pixels PER IMAGE) -- never of the batch size, the block tile or a timing --
   so the float32 summation order of every output element, hence every bit of a result, is the same whether an image is
   computed alone, inside a larger batch or on another rank.  gpp_conv2d_workspace_bytes: size of `partial` that any
   block tile of this layer may need (0 when the layer is not split). */
int gpp_conv2d_split_rule(const gpp_conv_desc* host_desc, int* split_k);
int gpp_conv2d_workspace_bytes(const gpp_conv_desc* host_desc, size_t* bytes);

/* Time the block-tile candidates of this layer on the device (iters launches each; the layer only rewrites its own
   output) and store the fastest in desc->tile_hint.  best_us (optional): its time per launch.  Synchronises the stream.
   Results do not depend on the tile (same K order per output element); split_k is used as given, never tuned. */
int gpp_conv2d_autotune(gpp_conv_desc* desc, int iters, void* stream, float* best_us);

/* The tile codes gpp_conv2d_autotune would time for this layer (count = how many there are; the first min(count, capacity)
   are written to tiles).  Any of them gives the same bytes; tests draw from this list at random (GPP_TUNE_RANDOM). */
int gpp_conv2d_tile_candidates(const gpp_conv_desc* host_desc, int* tiles, int capacity, int* count);

/* Fused tail of a ResNet bottleneck (keras_resnet bottleneck_2d, used at /root/reference/keras_retinanet_3D/models/
   resnet.py:88-93): the 3x3 conv "branch2b" (C -> C, C = 64 or 128, stride 1, pad 1, + bias + ReLU) and the 1x1 conv
   "branch2c" (C -> multiple of 128, + bias + residual + ReLU) in ONE launch; the intermediate map stays in LDS.
   conv3x3->out is not written.  Results are bit-identical to gpp_conv2d_igemm(conv3x3) + gpp_conv2d_igemm(conv1x1).
   tile_rows: 0 (= 128), 96, 128 or 160 output pixels per workgroup (the x3 types also 64: three workgroups per CU).  Other shapes,
   and GPP_F32: GPP_ERR_UNSUPPORTED. */
int gpp_bottleneck_tail(const gpp_conv_desc* conv3x3, const gpp_conv_desc* conv1x1, int tile_rows, void* stream);

/* A WHOLE bottleneck of the same graph in one launch (GPP_F16X3 / GPP_BF16X3 on pre-split maps): "branch2a" (1x1, C_in -> C, stride 1 or 2, + bias
   + ReLU), "branch2b" (3x3, C -> C, stride 1, pad 1, + bias + ReLU) and "branch2c" (1x1, C -> multiple of 128, + bias + shortcut + ReLU), C = 64 or
   128; both intermediate maps stay in LDS (a workgroup computes a tile of 8 x 14 output pixels and recomputes branch2a on its one-pixel halo).
   conv1x1_a->out and conv3x3_b->out are not written.  Results are bit-identical to the three gpp_conv2d_igemm launches (same K order and
   the same epilogue arithmetic per output element; range events counted once per stored group, as the three launches count them).  The
   shortcut is conv1x1_c->residual: a map a projection launch wrote, or the block's own input map -- an identity block (same pointer, offsets and
   pitches as conv1x1_a's input, stride 1, C_in = 4 C), whose shortcut rows are then taken from the LDS ring they pass through anyway and the map is
   read once (C = 64) / 1.25 times (C = 128) instead of twice.  tile: 0 = the library's choice (814 = 8 x 14 pixels, the only tile built);
   + 1000 forces the general form (the shortcut read from its map) on an identity block; + 10000 k: the odd tile rows start k microseconds late
   (an experiment).  Every map of the block must stay below 2 GiB per image.  Other shapes / types: GPP_ERR_UNSUPPORTED. */
int gpp_bottleneck_block(const gpp_conv_desc* conv1x1_a, const gpp_conv_desc* conv3x3_b, const gpp_conv_desc* conv1x1_c, int tile, void* stream);

/* The same launch for a block whose shortcut is a PROJECTION of its own input (res2a): conv1x1_proj ("branch1": 1x1, stride 1, C_in -> 4 C, + bias,
   no ReLU) is computed inside the launch from the input rows that pass through the LDS ring for branch2a, finished by its own epilogue (scale, bias,
   range check, split) in registers and added where gpp_bottleneck_block adds the shortcut map's values.  conv1x1_proj->out, conv1x1_a->out and
   conv3x3_b->out are not written; conv1x1_c->residual must be NULL.  Bit-identical to the four gpp_conv2d_igemm launches (branch2a, branch1,
   branch2b, branch2c), range events included.  GPP_ERR_UNSUPPORTED unless: one x3 type; C_in = C = 64 and C_out = 256 (res2a); both 1x1 layers on the input have
   stride 1, the same input pointer, offsets, pitch, C_in and sizes; every map behind the input is pre-split (the input itself pre-split or float32,
   the same for both of its readers); conv1x1_proj has no residual, ReLU, lists or guard.  tile as gpp_bottleneck_block's (0 or 814). */
int gpp_bottleneck_block_proj(const gpp_conv_desc* conv1x1_a, const gpp_conv_desc* conv3x3_b, const gpp_conv_desc* conv1x1_c,
                              const gpp_conv_desc* conv1x1_proj, int tile, void* stream);

/* GPP_F16X3 range ledger.  The half type ends at +-65504: an epilogue that stores an activation outside it (a finite value it has to
   clamp, an inf or a NaN) adds one event per 8-channel group to a device-side counter (one per device).  host_count (host pointer,
   may be NULL) receives the events since the last reset; reset != 0 clears the counter.  Synchronises the device.  Zero after a run
   means no activation of that run was altered by the type's range (models/retinanet.py: model.x3_range_events()). */
int gpp_x3_range_events(uint64_t* host_count, int reset);

/* The same counter WITHOUT a synchronisation: one tiny launch on `stream` copies the counter's value at that point of the stream
   into *device_count (8 bytes of device memory, or of page-locked host memory the device can write).  Enqueued behind a plan run,
   the value tells -- once the stream has reached it -- whether an activation of that run (or of any earlier one since the last
   reset) left the half range; models/retinanet.py reads it with the results it fetches anyway and re-runs an affected call at
   float32 (`on_range_event`), so that a clamped activation is never returned as a plausible wrong answer. */
int gpp_x3_range_snapshot(uint64_t* device_count, void* stream);

/* The same for a counter of the caller's (the slot its descriptors name in gpp_conv_desc.range_counter / gpp_stem_desc.range_counter; NULL = the
   library's per-device counter).  A caller that runs several GPP_F16X3 models, or one model from several streams, gives every plan its own
   8-byte slot: what one plan's launches count is then invisible to every other plan -- no spurious reaction, no missed one, whoever resets
   what (models/retinanet.py: Plan.range_slot). */
int gpp_x3_range_snapshot_of(const uint64_t* counter, uint64_t* device_count, void* stream);

/* Algorithmic FLOPs (2 * MACs) of one launch described by host_desc. */
int gpp_conv2d_flops(const gpp_conv_desc* host_desc, double* flops);

/* ------------------------------------------------------------------------------------------
 * DenseNet-121/169/201 backbone (keras.applications.densenet.DenseNet, used at /root/reference/keras_retinanet_3D/models/densenet.py:
 * 62-94).  A dense layer "convS_blockI" is _0_bn -> ReLU -> _1_conv (1x1) -> _1_bn -> ReLU -> _2_conv (3x3) -> concatenation; a
 * transition "poolS" is _bn -> ReLU -> _conv (1x1) -> AveragePooling2D(2, 2).  The BatchNormalization in front of each 1x1 belongs to the
 * CONSUMER of a concatenation, so it cannot be folded into any producer's weights: it runs as the prologue of the 1x1 conv.
 *
 * gpp_conv2d_preact: gpp_conv2d_igemm with every input activation x of channel c replaced by max(x * in_scale[c] + in_shift[c], 0)
 *     out = act( W . max(in (.) in_scale + in_shift, 0) + bias [+ residual] )
 *   in_scale / in_shift: [C_in] float32 device arrays, 16-byte aligned (the folded frozen BN: gamma / sqrt(var + eps), beta - mean * scale).
 *   Scope: 1 x 1, stride 1, pad 0 (a padded zero would become relu(in_shift)), an input map that is NOT pre-split (x3_split & GPP_X3_IN == 0;
 *   in_pitch > C_in reads a channel prefix of a wider map), C_in <= 4096; GPP_F32 / GPP_F16X3 / GPP_BF16X3 (other types:
 *   GPP_ERR_UNSUPPORTED).  The output may be pre-split (GPP_X3_OUT).  Same K order as gpp_conv2d_igemm, split-K by the same rule;
 *   tile_hint: 0 (128 x 128, 128 x 64 for C_out <= 64), 64064, 128064, 64128, 128128, 192128 -- every tile gives the same bytes. */
int gpp_conv2d_preact(const gpp_conv_desc* host_desc, const float* in_scale, const float* in_shift, void* stream);
int gpp_conv2d_preact_tile_candidates(const gpp_conv_desc* host_desc, int* tiles, int capacity, int* count);
/* times the candidates (iters launches each) and stores the fastest in desc->tile_hint; synchronises the stream */
int gpp_conv2d_preact_autotune(gpp_conv_desc* desc, const float* in_scale, const float* in_shift, int iters, void* stream, float* best_us);
/* ZeroPadding2D(pad) + MaxPooling2D(3, strides=2) 'pool1' (pad 0 or 1, symmetric): in (B, H, W, C) float32 dense, out pixel (b, y, x) at
   out + (b*Ho*Wo + y*Wo + x)*out_pitch, Ho = (H + 2 pad - 3)/2 + 1.  Padding never wins (-inf).  C % 4 == 0, out_pitch % 4 == 0. */
int gpp_maxpool3x3s2_pad_f32(const float* in, float* out, int B, int H, int W, int C, int pad, int out_pitch, void* stream);
/* AveragePooling2D(2, strides=2), valid: Ho = H/2, Wo = W/2 (floor); ((x00 + x01) + x10) + x11, then * 0.25.  Layout as above. */
int gpp_avgpool2x2_f32(const float* in, float* out, int B, int H, int W, int C, int out_pitch, void* stream);

/* ------------------------------------------------------------------------------------------
 * MobileNet (v1) backbone (keras.applications.mobilenet.MobileNet, include_top=False; csrc/mobilenet.hip), float32 NHWC storage.
 * Padding of both kernels: ZeroPadding2D(1) (symmetric) + 'valid', so H_out = (H - 1) / stride + 1 and output row y reads input rows
 * y * stride - 1 .. y * stride + 1 (NOT TensorFlow's 'same' window on an even side at stride 2).
 *
 * gpp_mobilenet_block: one depthwise-separable block as ONE launch; the depthwise map never reaches HBM
 *     out = relu6( W_pw . relu6( dw3x3(in, W_dw) + dw_bias ) + pw_bias ),  relu6(v) = min(max(v, 0), 6)
 *   in: (B, H, W) pixels of in_pitch floats, C_in channels read; out: (B, H_out, W_out) pixels of out_pitch floats, C_out written.
 *   dw_weight [9][C_in] float32 (tap dy * 3 + dx major, frozen BN folded in), dw_bias [C_in], pw_bias [C_out] float32.
 *   pw_weight [weight_rows][ceil(C_in / 32)][128 bytes]: row n = output channel n, zero rows up to weight_rows (a multiple of 256,
 *   >= C_out), zero channels up to the next multiple of 32; a 128-byte chunk is 32 float32 (GPP_F32) or [32 hi | 32 lo] 16-bit halves
 *   (GPP_F16X3 / GPP_BF16X3: hi = h(w), lo = h(w - hi); GPP_F16X3: w scaled by a per-channel power of two first, whose inverse is
 *   out_scale [C_out] float32 -- layers/mobilenet.py pack_pointwise).  Other dtypes: GPP_ERR_UNSUPPORTED.
 *   C_in % 4 == 0, C_out % 4 == 0, pitches % 4 == 0, every pointer 16-byte aligned, stride 1 or 2.
 *   The depthwise sum is float32 multiplies and adds in tap order, never contracted; the K order of the pointwise product is fixed
 *   (csrc/mobilenet.hip).  tile_hint: 0 (by C_out) or 128064, 64128, 128128, 64256 (pixels x channels): every tile gives the same bytes,
 *   and an image's bytes do not depend on the batch.  The depthwise result is at most 6: the f16x3 form needs no range counter.
 * gpp_mobilenet_stem: conv1 3x3 / 2, 3 -> C_out channels + folded BN + ReLU6; in (B, H, W, 3) float32 dense, weight [27][C_out] float32
 *   (tap (dy * 3 + dx) * 3 + input channel major), float32 multiplies and adds in tap order: the same bytes in every arithmetic mode. */
typedef struct gpp_mobilenet_block_desc {
    const float* in; const float* dw_weight; const float* dw_bias; const void* pw_weight; const float* pw_bias; const float* out_scale;
    float* out;
    int32_t dtype, B, H, W, C_in, C_out, stride, in_pitch, out_pitch, weight_rows, tile_hint, reserved;
} gpp_mobilenet_block_desc;
typedef struct gpp_mobilenet_stem_desc { const float* in; const float* weight; const float* bias; float* out; int32_t B, H, W, C_out, out_pitch, reserved; } gpp_mobilenet_stem_desc;
int gpp_mobilenet_block(const gpp_mobilenet_block_desc* host_desc, void* stream);
int gpp_mobilenet_block_tile_candidates(const gpp_mobilenet_block_desc* host_desc, int* tiles, int capacity, int* count);
/* times the candidates (iters launches each) and stores the fastest in desc->tile_hint; synchronises the stream */
int gpp_mobilenet_block_autotune(gpp_mobilenet_block_desc* desc, int iters, void* stream, float* best_us);
int gpp_mobilenet_stem(const float* in, const float* weight, const float* bias, float* out, int B, int H, int W, int C_out, int out_pitch,
                       void* stream);
/* the depthwise half of a block alone, its map stored (weight [9][C], the fused kernel's arithmetic): no plan uses it -- it exists so that
   tools/bench_mobilenet.py can time the two-launch form of a block against the fused one */
int gpp_mobilenet_depthwise(const float* in, const float* weight, const float* bias, float* out, int B, int H, int W, int C, int stride,
                            int in_pitch, int out_pitch, void* stream);

/* ------------------------------------------------------------------------------------------
 * ResNet stem and small element-wise helpers.
 * gpp_stem_conv7x7_bn_relu replaces keras_resnet's ZeroPadding2D(3) + conv1 (7x7, stride 2,
 * no bias) + bn_conv1 (frozen, eps 1e-5) + ReLU (instantiated at models/resnet.py:88-93):
 *   in (B, H, W, 3) float32 BGR mean-subtracted (utils/image.py:36-62), weight [7*7*3][64]
 *   float32 = Keras HWIO kernel with the BN scale folded in, bias [64] = folded BN shift,
 *   out (B, Ho, Wo, 64) of `dtype`, Ho = (H + 6 - 7)/2 + 1.  Float32 fmaf chain on the vector ALUs: the stem of the
 *   GPP_F32 (reference-precision) path; the 16-bit paths use the MFMA form below.
 * gpp_maxpool3x3s2_same replaces MaxPooling2D(3x3, stride 2, padding 'same') 'pool1'.
 * gpp_relu replaces Activation('relu') 'C6_relu' (models/retinanet.py:202).
 * ---------------------------------------------------------------------------------------- */
int gpp_stem_conv7x7_bn_relu(const float* in, const float* weight, const float* bias, void* out, int dtype,
                             int B, int H, int W, void* stream);
/* MFMA form of the stem (the one the model uses): float32 input and the packed weights are rounded to f16
 * (11-bit significand) on the fly, accumulated in float32 by v_mfma_f32_16x16x32_f16.  packed_weight_f16 is
 * the [64][232] f16 image that the HOST-side helper gpp_stem_pack_weights_f16 produces from the [147][64]
 * float32 folded kernel (14 848 elements = 29 696 bytes; both pointers of the helper are host pointers). */
int gpp_stem_pack_weights_f16(const float* host_weight_147x64, void* host_packed, size_t packed_bytes);
int gpp_stem_conv7x7_bn_relu_mfma(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                  int dtype, int B, int H, int W, void* stream);
int gpp_maxpool3x3s2_same(const void* in, void* out, int dtype, int B, int H, int W, int C, void* stream);
/* conv1 + bn_conv1 + ReLU + pool1 in ONE launch (GPP_BF16 / GPP_F16): out is the POOLED map (B, Hp, Wp, 64), Hp = (Ho + 1)/2;
 * the (B, Ho, Wo, 64) conv map is never written (137 MB at B = 8, 402 x 1333).  Bit-identical to
 * gpp_stem_conv7x7_bn_relu_mfma followed by gpp_maxpool3x3s2_same (the max is taken over the rounded conv values). */
int gpp_stem_pool_fused_mfma(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                             int dtype, int B, int H, int W, void* stream);
/* The stem of the float32-storage "x3" types (GPP_F16X3 / GPP_BF16X3 models): conv1 + bn_conv1 + ReLU on the matrix pipe at
 * (almost) float32 precision -- input pixels and weights split into two IEEE halves each, three matrix products per float32 product,
 * float32 output (B, Ho, Wo, 64).  packed_weight_x3 = what the HOST-side helper gpp_stem_pack_weights_f16x3 writes from the folded
 * [147][64] kernel: 2 * 64 * 232 halfs + 64 float32 (59 648 bytes).
 * The per-channel exponent is bounded to +-126 (scale and out_scale stay normal float32): a channel below 2^-113 packs finite, at fewer bits. */
int gpp_stem_pack_weights_f16x3(const float* host_weight_147x64, void* host_packed, size_t packed_bytes);
int gpp_stem_conv7x7_bn_relu_x3(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                int B, int H, int W, void* stream);
/* ... counting its range events (output values the half type cannot hold: the map is split -- and clamped -- by the layers that read it) into
 * the caller's 8-byte slot instead of the library's per-device counter (NULL = that one: the function above) */
int gpp_stem_conv7x7_bn_relu_x3_rc(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                   int B, int H, int W, uint64_t* range_counter, void* stream);
/* conv1 + bn_conv1 + ReLU + pool1 of the x3 types in ONE launch: out is the POOLED float32 map (B, Hp, Wp, 64); the (B, Ho, Wo, 64) float32
 * conv map (274 MB at B = 8, 402 x 1333) is never written.  Bit-identical to gpp_stem_conv7x7_bn_relu_x3_rc followed by
 * gpp_maxpool3x3s2_same(GPP_F32), and the range events of the conv map are counted as there (same count). */
int gpp_stem_pool_fused_x3(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                           int B, int H, int W, uint64_t* range_counter, void* stream);
/* Ragged batches: the forms of the six functions above for a batch whose images share a HEIGHT CLASS (Hp, W) -- the same pool1 map of Hp rows --
 * and differ in their own height H_b in [4 Hp - 3, 4 Hp].  `in` is a canvas (B, H, W, 3) with H = 4 Hp rows: image b occupies rows [0, H_b) of slot b,
 * and rows >= H_b are never read as data (they count as the zero padding below the image, whatever they hold).  heights = int32 [B] in DEVICE
 * memory, H_b per image: data, not a launch argument, so one plan and one captured graph serve every mix of heights.  Ho_b = (H_b - 1)/2 + 1 and
 * the pool's pad_top follow from H_b per image.  The unfused conv map is (B, 2 Hp, Wo, 64): image b's rows [0, Ho_b) are written, the rest is not
 * touched; gpp_maxpool3x3s2_same_ragged reads such a map (H = 2 Hp its rows; heights = the IMAGE heights, as for the stem) and writes (B, Hp, Wp, C).
 * For every image the result is bit-identical to the uniform function on that image alone (same taps, same accumulation order), and the x3 range
 * counter counts only conv values that exist (y < Ho_b).
 * Checked on the host before any launch: null pointers, sizes, alignment (heights: 4 bytes), and H == 4 Hp (the pool: H == 2 Hp), else
 * GPP_ERR_BAD_ARG / GPP_ERR_ALIGN.  The table itself cannot be read by the host: the caller checks 4 Hp - 3 <= H_b <= 4 Hp before upload (the
 * Python layer does), and the kernels clamp H_b into [1, H], so a bad table gives a wrong picture and never an access outside the canvas. */
int gpp_stem_conv7x7_bn_relu_ragged(const float* in, const float* weight, const float* bias, void* out, int dtype,
                                    int B, int H, int W, int Hp, const int32_t* heights, void* stream);
int gpp_stem_conv7x7_bn_relu_mfma_ragged(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                         int dtype, int B, int H, int W, int Hp, const int32_t* heights, void* stream);
int gpp_stem_conv7x7_bn_relu_x3_rc_ragged(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                          int B, int H, int W, int Hp, const int32_t* heights, uint64_t* range_counter, void* stream);
int gpp_maxpool3x3s2_same_ragged(const void* in, void* out, int dtype, int B, int H, int W, int C, int Hp,
                                 const int32_t* heights, void* stream);
int gpp_stem_pool_fused_mfma_ragged(const float* in, const void* packed_weight_f16, const float* bias, void* out,
                                    int dtype, int B, int H, int W, int Hp, const int32_t* heights, void* stream);
int gpp_stem_pool_fused_x3_ragged(const float* in, const void* packed_weight_x3, const float* bias, float* out,
                                  int B, int H, int W, int Hp, const int32_t* heights, uint64_t* range_counter, void* stream);
/* dtype GPP_BF16X3 = a pre-split map (gpp_conv_desc.x3_split): ReLU on the [hi | lo] pairs (count in float32-sized elements, a
   multiple of 32) */
int gpp_relu(const void* in, void* out, int dtype, int64_t count, void* stream);
/* batched form: image b reads `count` elements at in + b*in_bstride, writes out + b*out_bstride */
int gpp_relu_strided(const void* in, int64_t in_bstride, void* out, int64_t out_bstride, int dtype, int B,
                     int64_t count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Image preprocessing: uint8 BGR frames (B, H, W, 3) -> float32 (B, Ho, Wo, 3),
 * ImageNet mean subtracted per channel, then bilinear resize.  Replaces the host-side
 * utils/image.py:36-62 (preprocess_image) + :174-200 (resize_image -> cv2.resize INTER_LINEAR).
 * y0/y1/wy (Ho entries) and x0/x1/wx (Wo entries) are the interpolation taps: source indices and the
 * float32 weight of the second one, as cv2 derives them from the scale (half-pixel centres, border
 * replicated); device arrays, computed once per input shape by the host.
 * ---------------------------------------------------------------------------------------- */
int gpp_preprocess_u8_bgr(const uint8_t* frames, float* out, const int32_t* y0, const int32_t* y1, const float* wy,
                          const int32_t* x0, const int32_t* x1, const float* wx, int B, int H, int W, int Ho, int Wo,
                          float mean_b, float mean_g, float mean_r, void* stream);
/* The ragged form (see the ragged stem above): frames of different raw sizes that resize into one height class.  frames = a uint8 canvas of
 * B slots of H x W x 3 bytes (H, W = the largest raw height and width); frame b is stored DENSELY, h_b x w_b x 3 bytes from the start of its
 * slot; raw_hw = int32 [B][2] = (h_b, w_b); heights = int32 [B] = the resized heights H_b; y0/y1/wy are [B][Ho] and x0/x1/wx [B][Wo], image b's
 * row being the taps of that image alone (entries of rows >= H_b are not read).  out = the float32 canvas (B, Ho, Wo, 3) with Ho = 4 Hp: rows
 * [0, H_b) of image b are bit-identical to gpp_preprocess_u8_bgr on that frame alone, rows >= H_b are written as zero.  All tables are device
 * arrays; sizes and taps are clamped into the slot.  Null pointer, bad size, Ho != 4 Hp: GPP_ERR_BAD_ARG; a table not 4-byte aligned: GPP_ERR_ALIGN. */
int gpp_preprocess_u8_bgr_ragged(const uint8_t* frames, float* out, const int32_t* raw_hw, const int32_t* heights,
                                 const int32_t* y0, const int32_t* y1, const float* wy, const int32_t* x0, const int32_t* x1, const float* wx,
                                 int B, int H, int W, int Hp, int Ho, int Wo, float mean_b, float mean_g, float mean_r, void* stream);

/* ------------------------------------------------------------------------------------------
 * Detection decode: sigmoid, orientation fold, score threshold, NMS, top-k, box / dimension
 * decode, -1 padding.  Replaces models/retinanet.py:72-73 (sigmoid), layers/_misc.py:133-141
 * + backend/common.py:43-81 (RegressBoxes), layers/_misc.py:186-187 + backend/common.py:23-40
 * (RegressDims) and layers/filter_detections.py:18-189 on its default path (nms=True,
 * class_specific_filter=True, orientation_specific_filter=False, one class).
 *
 *   cls_logits     (B, n_anchors, 8)  f32  pre-sigmoid classification head output
 *   regression     fused_layout == 0: (B, n_anchors, 12) f32 as the reference concatenates it
 *                  (retinanet.py:112-124); fused_layout == 1: (B, n_anchors/A, 12*A) f32, per
 *                  pixel [op1: 4A | op2: 2A | op3: 2A | op4: 2A | op5: 2A] (one fused conv)
 *   regression_dim (B, n_anchors, 3)  f32
 *   anchors        (n_anchors, 4)     f32  x1 y1 x2 y2 (layers/_misc.py:24-87), 16-byte aligned
 *   boxes (B, max_det, 12) dims (B, max_det, 3) scores (B, max_det) f32,
 *   labels / orientations (B, max_det) i32; rows past the survivors are -1
 *   anchor_index   (B, max_det) i32 anchor id of each detection (may be NULL; not a reference output)
 *   counts         (B) i32 number of anchors above score_thr per image (may be NULL)
 *   workspace      gpp_detect_workspace_bytes() bytes, 16-byte aligned
 * Reference constants: score_thr 0.05, iou_thr 0.5, max_det 100 (filter_detections.py:26-28).
 * ---------------------------------------------------------------------------------------- */
int gpp_detect_workspace_bytes(int B, int64_t n_anchors, size_t* bytes);

int gpp_detect_f32(const float* cls_logits, const float* regression, const float* regression_dim,
                   const float* anchors, int B, int64_t n_anchors, int num_base_anchors, int fused_layout,
                   float score_thr, float iou_thr, int max_det,
                   float* boxes, float* dims, float* scores, int32_t* labels, int32_t* orientations,
                   int32_t* anchor_index, int32_t* counts,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The same work as three separately enqueueable stages (bit mask; gpp_detect_f32 = all three, in this order):
 *   GPP_DETECT_CANDIDATES  sigmoid + fold + threshold -> candidate keys      reads cls_logits only
 *   GPP_DETECT_SELECT      sort + greedy NMS -> survivors' keys              reads the keys + corner regressions
 *   GPP_DETECT_EMIT        full decode of the survivors, -1 padding           reads every head tensor
 * so that a caller can start the (latency-bound, one workgroup per image) selection as soon as the classification
 * and regression heads are done and overlap it with the dimension head (models/retinanet.py:128-167).  All stages
 * take the full argument list; state passes through `workspace`. */
#define GPP_DETECT_CANDIDATES 1
#define GPP_DETECT_SELECT 2
#define GPP_DETECT_EMIT 4
int gpp_detect_stages_f32(int stages, const float* cls_logits, const float* regression, const float* regression_dim,
                          const float* anchors, int B, int64_t n_anchors, int num_base_anchors, int fused_layout,
                          float score_thr, float iou_thr, int max_det,
                          float* boxes, float* dims, float* scores, int32_t* labels, int32_t* orientations,
                          int32_t* anchor_index, int32_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The pixels the decode will read: from the candidate keys of GPP_DETECT_CANDIDATES (still unsorted in `workspace`), per pyramid level the
 * ascending list of the pixels b * level_pixels[l] + p that carry at least one candidate anchor (anchor a of an image lies on pixel
 * a / num_base_anchors of the image's levels laid back to back).  The lists are what gpp_conv_desc.gather_rows / gather_counts take: the head
 * output layers then run on those pixels only.  Built through one bit per pixel, so a list is a function of the candidate SET, not of the order
 * the candidates' atomics arrived in.  Two small launches on `stream`.
 *   workspace        the workspace of gpp_detect_stages_f32 / gpp_detect_osf_f32 after its candidate stage; lists_per_image 1 or 4 (osf)
 *   level_pixels     H_l * W_l of every level, n_levels <= GPP_MAX_GROUPS, their sum * num_base_anchors == n_anchors
 *   bitmap           uint32, sum over the levels of ceil(B * level_pixels[l] / 32) words; zero before the first call, left zero by every call
 *   rows             int32 [B * sum(level_pixels)]: level l's list starts at B * (pixels of the levels before l)
 *   counts           int32 [GPP_MAX_GROUPS + 1]: the length of every level's list, then their sum
 *   flag             int32 [1]: 1 when the sum exceeds max_rows, else 0 (gpp_conv_desc.guard of the gathered and of the dense launch)
 * Null pointer, bad size: GPP_ERR_BAD_ARG; nothing launched.  B == 0: GPP_OK. */
typedef struct gpp_pixel_list_desc {
    const void* workspace; uint32_t* bitmap; int32_t* rows; int32_t* counts; int32_t* flag;
    int64_t n_anchors;
    int32_t B, num_base_anchors, lists_per_image, n_levels, max_rows, reserved;
    int32_t level_pixels[GPP_MAX_GROUPS]; int32_t reserved2;
    /* the DILATED lists (NULL / 0 = none): every listed pixel and its eight neighbours inside its own image and level -- what a 3 x 3, pad 1
       layer on the lists above reads, and so what the layer in front of it has to write.  Same layout as bitmap / rows / counts; level_width[l] =
       W_l (a divisor of level_pixels[l]).  dilated_flag = flag | (sum of the dilated counts > dilated_max_rows): when the reader runs dense it
       reads every row, so its producer runs dense too.  All four pointers or none */
    uint32_t* dilated_bitmap; int32_t* dilated_rows; int32_t* dilated_counts; int32_t* dilated_flag;
    int32_t level_width[GPP_MAX_GROUPS]; int32_t dilated_max_rows;
} gpp_pixel_list_desc;
int gpp_detect_pixel_lists(const gpp_pixel_list_desc* host_desc, void* stream);

/* The rows the regression tower's layers 2 and 1 have to write, straight from the logits: no keys, no workspace of the candidate pass, four small
 * launches on ONE stream (the caller's, behind the layer that writes the logits: gpp_conv_desc.lists_after).
 *   marks            one bit per (level, image, pixel), the layout of gpp_pixel_list_desc.bitmap: set iff one of the pixel's num_base_anchors anchors
 *                    is a candidate by the decision GPP_DETECT_CANDIDATES makes at score_thr (the same device functions) -- the pixel set of
 *                    gpp_detect_pixel_lists' undilated lists
 *   radius1/2/3      the 3 x 3, 5 x 5 and 7 x 7 dilations of the marks inside the pixel's own image and level (level_width[l] = W_l): what the
 *                    output layer, layer 3 and layer 2 read.  Every word of the four maps is written whole, whatever it held; a map that
 *                    is compacted (radius2; radius3 with layer 1's lists) is zero again when the call has run
 *   rows2 / counts2  the radius-2 map as ascending per-level lists with their lengths and the sum, the layout of gpp_conv_desc.gather_rows /
 *                    gather_counts: the rows of layer 2.  rows1 / counts1: the radius-3 map, the rows of layer 1 (all three of rows1, counts1,
 *                    flag1 NULL: layer 2 only)
 *   stats            int32 [4]: |marks|, |radius 1|, f3, flag2.  f3 = (|marks| > max_rows) | (|radius 1| > tower_max_rows) is what the candidate
 *                    pass's lists will decide for layer 3 (gpp_pixel_list_desc.dilated_flag)
 *   flag2, flag1     int32 [1] each, 1 = dense: flag2 = f3 | (|radius 2| > deep_max_rows), flag1 = flag2 | (|radius 3| > deep_max_rows) -- a layer
 *                    whose reader runs dense runs dense, by construction
 *   radius4 / rows0 / counts0 / flag0 / stats0   (all five NULL: none, and the call is the one above byte for byte.  All five or none; they need
 *                    rows1 / counts1 / flag1.)  The 9 x 9 dilation, written in the same pass as the other three and compacted by a third workgroup
 *                    of the compaction launch into the rows of LAYER 0's regression slice (gpp_conv_desc.conv_after), which layer 1 reads on the
 *                    halo of its own rows; flag0 = flag1 | (|radius 4| > deep_max_rows).  stats0: int32 [1], flag1 as the statistics launch
 *                    computes it (the third compaction does not wait for the second); stats keeps its four words
 * Null pointer, bad size, num_base_anchors > 64, reserved != 0: GPP_ERR_BAD_ARG; nothing launched.  B == 0: GPP_OK.
 * gpp_detect_deep_lists_register keeps a copy of a descriptor in the library and hands out a handle > 0 for gpp_conv_desc.lists_after (a number,
 * not an address: a conv descriptor holds no host pointer); gpp_detect_deep_lists_release gives it back. */
typedef struct gpp_deep_list_desc {
    const float* cls_logits;
    uint32_t* marks; uint32_t* radius1; uint32_t* radius2; uint32_t* radius3;
    int32_t* rows2; int32_t* counts2; int32_t* flag2;
    int32_t* rows1; int32_t* counts1; int32_t* flag1;
    int32_t* stats;
    int64_t n_anchors;
    int32_t B, num_base_anchors, n_levels, max_rows, tower_max_rows, deep_max_rows;
    float score_thr; int32_t reserved;
    int32_t level_pixels[GPP_MAX_GROUPS]; int32_t level_width[GPP_MAX_GROUPS];
    uint32_t* radius4; int32_t* rows0; int32_t* counts0; int32_t* flag0; int32_t* stats0;
} gpp_deep_list_desc;
int gpp_detect_deep_lists(const gpp_deep_list_desc* host_desc, void* stream);
int gpp_detect_deep_lists_register(const gpp_deep_list_desc* host_desc, int32_t* handle);
int gpp_detect_deep_lists_release(int32_t handle);
/* gpp_detect_deep_lists of the descriptor a handle names (check_only != 0: whether somebody holds the handle, nothing launched) */
int gpp_detect_deep_lists_run(int32_t handle, int check_only, void* stream);

/* orientation_specific_filter=True (layers/filter_detections.py:84-98, a non-default argument of models.load_model): threshold
 * and NMS once per orientation on that orientation's folded score, the four survivor lists concatenated in orientation
 * order, then the common top-k; an anchor may be reported once per orientation.  Same arguments as gpp_detect_f32; its own
 * (4x larger) workspace; at most 16 images per call. */
int gpp_detect_osf_workspace_bytes(int B, int64_t n_anchors, size_t* bytes);
int gpp_detect_osf_f32(const float* cls_logits, const float* regression, const float* regression_dim,
                       const float* anchors, int B, int64_t n_anchors, int num_base_anchors, int fused_layout,
                       float score_thr, float iou_thr, int max_det,
                       float* boxes, float* dims, float* scores, int32_t* labels, int32_t* orientations,
                       int32_t* anchor_index, int32_t* counts,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The eight result arrays -> one (B, D, 35) float32 tensor [12 box | 3 dim | score | label | orientation | 12 keypoints |
 * 4 plane | residual]: the unit of the per-step exchange between the ranks of a node (one all-gather). */
int gpp_pack_detections(const float* boxes, const float* dims, const float* scores, const int32_t* labels,
                        const int32_t* orientations, const float* keypoints, const float* keyplanes,
                        const float* residuals, int B, int D, float* packed, void* stream);

/* ------------------------------------------------------------------------------------------
 * 6-DoF pose and KITTI fields of the detections on the device (csrc/pose.hip): what bin/run_network.py does on the host after
 * predict_on_batch -- scale correction and selection (reference run_network.py:113-135), pose from the 3-D keypoints (:137-247),
 * cuboid corners and the KITTI fields (:298-330).  One thread per detection; the float32 inputs are read once, every step is
 * float64, and each value is rounded to float32 once, where it is stored.
 *
 *   boxes (B, D, 12), dims (B, D, 3), scores (B, D), labels (B, D), orientations (B, D), keypoints (B, D, 4, 3),
 *   residuals (B, D): the outputs of gpp_detect_f32 / gpp_poll_f32.
 *   frame_info (B, 3) float32, device: per image the image scale, the raw image's height and its width.
 *   rows (B, D, GPP_POSE_COLS) float32: row d of image b belongs to detection d (no compaction).  A row whose score is not above
 *   score_thr, or whose orientation is -1 (padding), is -1 in every column and is not counted in counts[b].
 *
 *   columns   content
 *    0 -  3   box x1 y1 x2 y2 divided by the scale
 *    4 - 11   2-D keypoints xl yl xm ym xr yr xt yt divided by the scale
 *   12 - 15   score, label, orientation class, polling residual (passed through)
 *   16 - 18   dimensions h w l: h = |X_t - X_m|, l = |X_s - X_m| (X_s = X_l for orientation 0 and 3, X_r for 1 and 2), w the network's
 *   19 - 21   location (centre of the bottom face)
 *   22 - 24   rotation vector (axis * angle) of the polar factor U V^T of [x y z]
 *   25        alpha, in [-pi, pi)
 *   26 - 29   the box clipped to the raw image: max(x1, 0) max(y1, 0) min(x2, width) min(y2, height)
 *   30 - 32   KITTI height (corner Y max - min), KITTI y (corner Y max), r_y in [-pi, pi)
 *   33 - 35   0
 *
 *   A KITTI result line is columns 25, 26-29, 30, 17, 18, 19, 31, 21, 32, 12 in that order.
 *   A detection with a zero-length edge (h = 0 or l = 0: [x y z] is not finite), or one whose two edges are parallel ([x y z] is singular),
 *   has NaN in columns 19-25 and 30-32; its other columns and every other row are as usual.
 *   Null pointer or negative size: GPP_ERR_BAD_ARG, nothing launched.  B * D == 0: GPP_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
#define GPP_POSE_COLS 36
int gpp_pose_f32(const float* boxes, const float* dims, const float* scores, const int32_t* labels,
                 const int32_t* orientations, const float* keypoints, const float* residuals,
                 const float* frame_info, int B, int D, float score_thr,
                 float* rows, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Matching of detections to labels for the evaluation on the device (csrc/eval.hip): what utils/eval.py does
 * on the host with the outputs of one image -- selection and order (_image_rows; reference utils/eval.py:93-118) and the greedy
 * assignment inside every (class, orientation) bin (_match_bin; :207-226) -- restated per detection.  One launch, one workgroup per
 * image, one thread per detection.
 *
 *   boxes (B, D, 12), dims (B, D, 3), scores (B, D) float32, labels (B, D), orientations (B, D) int32: the outputs of gpp_detect_f32
 *   as a plan leaves them (padding rows are -1), in any order.
 *   scales (B) float32, device: the image scale of every image.
 *   annotations (B, A, GPP_EVAL_ANN_COLS) float64, device: the rows of KittiGenerator.load_annotations, padded to A rows per image --
 *   0-3 box, 4-11 keypoint pixels, 12-14 h w l, 15 class, 16 orientation; ann_counts (B) int32: the rows of image b that count
 *   (clamped to [0, A]).  A == 0: annotations may be null.
 *   table (B, D, 3) int32, row d of image b belongs to detection d: bin, hit, annotation row.
 *   errors (B, D, GPP_EVAL_ERR_COLS) float64; counts (B) int32: the selected detections of the image.
 *
 *   selected    score > score_thr (strict) and rank < max_detections; rank = the entries of the image with a higher score, or an equal
 *               score and a lower index (the stable descending order; computed here, the input need not be sorted).
 *               A detection that is not selected has -1 in all three table columns and zeros in its errors.
 *   bin         4 * label + orientation if 0 <= label < num_classes and 0 <= orientation < 4, else -1 (such a detection is selected
 *               and counted, claims nothing and is no hit).  An annotation's bin likewise, from columns 15 and 16.
 *   geometry    box columns 0-11 divided by the scale in float32, then widened to float64; dims widened.
 *   IoU         float64, the operation sequence of utils/anchors.compute_overlap with the union clamped to DBL_EPSILON, no contraction.
 *   claim       the FIRST annotation of the detection's bin with the largest IoU (column 2; -1 without one: a miss).
 *   hit         the claimed IoU is >= iou_thr and the detection has the lowest rank among the selected detections that claim the same
 *               annotation with IoU >= iou_thr (column 1: 1 or 0).
 *   errors      of a hit: |detection - annotation| over the 8 keypoint pixels (divided by the scale), then h w l; zeros otherwise.
 *
 *   D <= GPP_EVAL_MAX_DETECTIONS and A <= GPP_EVAL_MAX_ANNOTATIONS, beyond: GPP_ERR_UNSUPPORTED.  Null pointer or negative size or
 *   count: GPP_ERR_BAD_ARG, nothing launched.  B * D == 0: GPP_OK, nothing launched.  A == 0 or a count of 0: every selected
 *   detection is a miss.  Finite inputs are the contract.
 * ---------------------------------------------------------------------------------------- */
#define GPP_EVAL_MAX_DETECTIONS 1024
#define GPP_EVAL_MAX_ANNOTATIONS 1024
#define GPP_EVAL_ANN_COLS 17
#define GPP_EVAL_ERR_COLS 11
int gpp_eval_match_f32(const float* boxes, const float* dims, const float* scores, const int32_t* labels,
                       const int32_t* orientations, const float* scales, const double* annotations,
                       const int32_t* ann_counts, int B, int D, int A, int num_classes, float score_thr,
                       int max_detections, double iou_thr, int32_t* table, double* errors, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * KITTI's object benchmark on the device (csrc/kitti_eval.hip; DESIGN.md section 4.17 is the specification, a restatement of the
 * devkit's evaluate_object.cpp -- parity with the devkit itself is UNPINNED; utils/kitti_eval.py is the host form): AP of the image box,
 * the bird's-eye-view (BEV) box and the 3-D box at Easy / Moderate / Hard, and AOS, of the rows of gpp_pose_f32 against label_2 rows.
 * Two entry points: the overlaps of every (detection, label) pair once, then the matching of every image, called once without
 * thresholds (pass 1: the true positives' scores, from which the host takes the 41 recall thresholds) and once with them (pass 2).
 *
 *   rows (B, D, GPP_POSE_COLS) float32, device: the rows of gpp_pose_f32.  A row is a detection iff its column 14 is >= 0; the columns of
 *   the KITTI line are read: 12 score, 25 alpha, 26-29 box, 30 h, 17 w, 18 l, 19 x, 31 y, 21 z, 32 r_y.  Every detection is a Car.
 *   labels (B, A, GPP_KITTI_LABEL_COLS) float64, device: column 0 the type code (0 Car, 1 Van, 2 DontCare, 3 anything else), columns
 *   1-14 the numeric fields of a label_2 line (truncation, occlusion, alpha, box x1 y1 x2 y2, h w l, x y z, r_y), column 15 zero.
 *   label_counts (B) int32, device: the rows of image b that count (clamped to [0, A]).  A == 0: labels and overlaps may be null.
 *
 * gpp_kitti_overlaps_f64: one thread per (detection, label) pair.
 *   overlaps (B, 4, D, A) float64: plane 0 the image IoU (no "+1"; a non-positive width or height of the intersection: 0), plane 1 the
 *   BEV IoU (the rectangle with corners (+-l/2, +-w/2) placed by X = cos(ry) x + sin(ry) z + tx, Z = -sin(ry) x + cos(ry) z + tz; the
 *   intersection of the two quadrilaterals by Sutherland-Hodgman clipping, up to 8 vertices in LDS), plane 2 the 3-D IoU (BEV
 *   intersection times max(0, min(y_d, y_g) - max(y_d - h_d, y_g - h_g)) over the union of the volumes), plane 3 the image intersection
 *   over the detection's area (the DontCare form).  An overlap with a NaN operand is NaN (a pose row has NaN 3-D fields when its
 *   keypoints are singular).  Entries of padding rows and of labels beyond the count are 0.  Positive sides are the contract.
 *
 * gpp_kitti_stats_f64: one workgroup per image, one thread per (metric, difficulty, threshold); metric 0 image, 1 BEV, 2 3-D;
 * difficulty 0 Easy (box height >= 40, occlusion <= 0, truncation <= 0.15), 1 Moderate (25, 1, 0.30), 2 Hard (25, 2, 0.50).
 *   min_overlap: 3 doubles on the HOST, one per metric (KITTI's Car: 0.7 each); a match needs overlap > min_overlap (strict).
 *   thresholds (3, 3, T) float32 and n_thresholds (3, 3) int32, device -- or thresholds == null for pass 1 (T is then ignored but checked).
 *   pass 1 writes tp_scores (B, 3, 3, A) float32 -- the score of the detection that label a takes as a true positive, NaN where it takes
 *   none -- and n_gt (B, 3, 3) int32, the labels that count.  Each label takes the free detection of the highest score (the first of equals).
 *   pass 2 writes stats (B, 3, 3, T, 3) int32 -- tp, fp, fn at threshold k; zeros for k >= n_thresholds -- and similarity (B, 3, 3, T)
 *   float64, the sum of (1 + cos(alpha_gt - alpha_det)) / 2 over the true positives in label order (metric 0; 0 for the others).
 *   Detections with score < threshold (float32 against float32) are out; each label takes the free detection of the largest overlap,
 *   a detection too low for the difficulty only when nothing else offers; a label that does not count (a Van, a Car too hard for the
 *   difficulty) or a too-low detection makes the pair neither tp nor fp; for metric 0 a left-over detection in a DontCare box is no fp.
 *   The per-image outputs are summed by the host in image order: no floating-point atomics, the result is a function of the inputs.
 *
 *   D <= GPP_KITTI_MAX_DETECTIONS and A <= GPP_KITTI_MAX_LABELS (the assigned set is a 128-bit mask), beyond: GPP_ERR_UNSUPPORTED.
 *   Null pointer, negative size, T > GPP_KITTI_MAX_THRESHOLDS: GPP_ERR_BAD_ARG, nothing launched.  B * D == 0: GPP_OK, nothing launched.
 *   A == 0 or a count of 0: every detection above the threshold and high enough is an fp.
 * ---------------------------------------------------------------------------------------- */
#define GPP_KITTI_MAX_DETECTIONS 128
#define GPP_KITTI_MAX_LABELS 128
#define GPP_KITTI_MAX_THRESHOLDS 41
#define GPP_KITTI_LABEL_COLS 16
int gpp_kitti_overlaps_f64(const float* rows, const double* labels, const int32_t* label_counts, int B, int D, int A,
                           double* overlaps, void* stream);
int gpp_kitti_stats_f64(const float* rows, const double* labels, const int32_t* label_counts, const double* overlaps,
                        const double* min_overlap, const float* thresholds, const int32_t* n_thresholds, int B, int D, int A, int T,
                        float* tp_scores, int32_t* n_gt, int32_t* stats, double* similarity, void* stream);

/* ------------------------------------------------------------------------------------------
 * Suppression of duplicate cuboids on the device (csrc/cuboid_nms.hip; DESIGN.md section 4.26 is the specification,
 * utils/cuboid_nms.py the host form): a greedy non-maximum suppression of the rows of gpp_pose_f32 by the overlap of the cuboids
 * themselves -- in the bird's-eye view or in 3-D -- where the decode's NMS judges image rectangles.  One launch, one workgroup per image.
 *
 *   rows_in, rows_out (B, D, GPP_POSE_COLS) float32, device: the rows of gpp_pose_f32.  rows_out == rows_in is allowed (the form a plan
 *   uses); otherwise the two do not overlap.  A workgroup reads all it needs of its image before it writes any of it.
 *   live        a row is live iff its column 14 is >= 0.
 *   rank        live rows by (column 12 descending, row index ascending), computed here: the rows need not arrive sorted (rows built
 *               from labels all score 1).  A NaN score ranks as -infinity.
 *   overlap     of the live rows i < j: row i in the place of gpp_kitti_overlaps_f64's detection, row j in the place of its label --
 *               the fields w 17, l 18, x 19, z 21, r_y 32 (3-D also h 30, y 31), the same corner order, placement, clipping (row i's
 *               rectangle against row j's edges), area sum and height term, operation for operation (csrc/rot_iou.h); overlap(j, i) is
 *               overlap(i, j).  A NaN operand gives a NaN overlap, which suppresses nothing and is suppressed by nothing.
 *   metric      GPP_CUBOID_NMS_BEV: plane 1 of gpp_kitti_overlaps_f64; GPP_CUBOID_NMS_3D: plane 2.
 *   greedy      in rank order a row is kept iff no already KEPT row overlaps it by more than iou_thr (strict); a suppressed row
 *               suppresses nothing.
 *   rows_out    a suppressed row is -1 in all its columns -- the padding every reader skips; kept rows and padding rows are copied bit
 *               for bit (in place: left alone).
 *   counts (B) int32: the kept rows of image b.
 *   suppressor (B, D) int32: the row index of the kept row that removed row d -- of several, the first in rank order; -1 for kept rows
 *               and padding rows.
 *
 *   A pair whose centres lie further apart than the sum of the two half-diagonals times 1 + 1/32 has an empty intersection and is not
 *   clipped; the gate changes no overlap (section 4.26 has the argument).
 *   D <= GPP_KITTI_MAX_DETECTIONS (the kept set is a 128-bit mask, as the assigned set of gpp_kitti_stats_f64), beyond:
 *   GPP_ERR_UNSUPPORTED.  iou_thr outside (0, 1) or NaN, a metric other than the two: GPP_ERR_BAD_ARG.  Null pointer or negative size:
 *   GPP_ERR_BAD_ARG, nothing launched.  B * D == 0: GPP_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
#define GPP_CUBOID_NMS_BEV 0
#define GPP_CUBOID_NMS_3D 1
int gpp_cuboid_nms_f64(const float* rows_in, int B, int D, int metric, double iou_thr,
                       float* rows_out, int32_t* counts, int32_t* suppressor, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tracking of cuboids across frames on the device (csrc/track.hip; DESIGN.md section 4.28 is the specification, utils/track.py the
 * host form): a greedy association of the rows of gpp_pose_f32 of one frame with the cuboids carried over from the frames before, and a
 * fixed-gain (alpha-beta) filter on each carried cuboid.  One launch, one workgroup per sequence, which walks its frames in order.
 *
 *   rows_in, rows_out (N, D, GPP_POSE_COLS) float32, device: the rows of N frames.  rows_out == rows_in is allowed; otherwise the two do
 *               not overlap.  A workgroup reads all it needs of a frame before it writes any of that frame.
 *   seq_start   (S + 1) int32 on the HOST, 0 <= seq_start[0] <= ... <= seq_start[S] <= N: the frames of sequence s are
 *               [seq_start[s], seq_start[s + 1]) in time order.  Frames outside every sequence are not touched.
 *   state_in, state_out (S, gpp_track_state) on the device, 8-byte aligned; they may be the same buffer, otherwise they do not overlap.
 *               A state of all zero bytes is the empty tracker.  The host may read a state back (gpp_track_state below).
 *   frame step  all float64, every operation separate.  For the rows of one frame:
 *     1 predict    every occupied slot: x += vx, y += vy, z += vz (velocity is per frame step; there is no time difference).
 *     2 rows       a row is live iff its column 14 is >= 0; a live row with a NaN among the columns 17 18 19 21 30 31 32 is blind: never
 *                  matched, never born, id -1.
 *     3 candidates slot t against live, non-blind row d.  GPP_TRACK_BEV / GPP_TRACK_3D: the overlap of gpp_kitti_overlaps_f64 (plane 1 /
 *                  plane 2) with the slot's predicted cuboid in the place of the detection and the row in the place of the label
 *                  (csrc/rot_iou.h, the gate of gpp_cuboid_nms_f64 included); a candidate iff overlap > threshold (strict); the larger
 *                  overlap is better.  GPP_TRACK_DIST: q = dx dx + dz dz between the centres on the ground plane; a candidate iff
 *                  q < threshold * threshold; the smaller q is better.
 *     4 greedy     candidates best first, ties to the smaller slot, then to the smaller row; taken iff slot and row are both free.
 *     5 update     of a matched pair, per component of x y z: r = row - predicted, position = predicted + a r, velocity += b r;
 *                  h (30), w (17), l (18): s += c (row - s); r_y: delta = wrap(row - slot) in [-pi, pi), delta -= pi if delta >= pi / 2,
 *                  delta += pi if delta < -pi / 2 (a detection facing the other way is read as facing the track's), r_y = wrap(r_y +
 *                  a delta), the wrap of gpp_pose_f32; hits += 1, misses = 0, score = the row's column 12.
 *     6 deaths     an occupied, unmatched slot: misses += 1; freed (all its fields 0) iff misses > max_age.
 *     7 births     after the deaths: live, non-blind, unmatched rows with column 12 >= birth_score (a NaN score is not), in ascending row
 *                  order, each into the lowest free slot: id = next_id++, the row's fields, velocity 0, hits 1, misses 0.  No free slot:
 *                  id -1 and dropped += 1.
 *   track_ids   (N, D) int32: the id of the slot the row matched or was born into; -1 for padding, blind and unborn rows.
 *   track_hits  (N, D) int32: that slot's hits after the step; 0 where the id is -1.
 *   rows_out    smooth == 0: a bit copy.  smooth == 1: in rows that carry an id the columns 19 31 21 30 17 18 32 are the slot's
 *               x y z h w l r_y after the step, each rounded to float32 once, and column 25 is wrap(r_y - atan2(x, z)); all else a bit copy.
 *   workspace   gpp_track_workspace_bytes(S) bytes on the device, 8-byte aligned: seq_start's copy and, per sequence, the
 *               GPP_TRACK_MAX_TRACKS x GPP_KITTI_MAX_DETECTIONS float64 table of the frame's candidates and its transpose (128 KiB each:
 *               they do not fit into LDS beside the clipping buffers).  Nothing in it survives the call.
 *
 *   GPP_ERR_BAD_ARG, nothing launched: an unknown metric; a BEV / 3-D threshold outside [0, 1); a DIST threshold that is not finite and
 *   positive; gain_a outside (0, 1]; gain_b or gain_c outside [0, 1]; max_age < 0; smooth other than 0 or 1; reserved != 0; a NaN in any
 *   of them or in birth_score; a seq_start that is not monotone inside [0, N]; a null pointer; a negative size.  A short workspace:
 *   GPP_ERR_WORKSPACE.  D > GPP_KITTI_MAX_DETECTIONS: GPP_ERR_UNSUPPORTED.  N * D == 0 or S == 0: GPP_OK, state_in is copied to state_out
 *   and nothing else is written.
 * ---------------------------------------------------------------------------------------- */
#define GPP_TRACK_BEV 0
#define GPP_TRACK_3D 1
#define GPP_TRACK_DIST 2
#define GPP_TRACK_MAX_TRACKS 128
#define GPP_TRACK_FIELDS 10              /* x y z r_y h w l vx vy vz */
typedef struct gpp_track_state {
    int32_t id1[GPP_TRACK_MAX_TRACKS];                        /* id + 1 of the slot's track; 0: the slot is free */
    int32_t hits[GPP_TRACK_MAX_TRACKS];                       /* frames in which the track was matched, its birth included */
    int32_t misses[GPP_TRACK_MAX_TRACKS];                     /* frames since it was last matched */
    float score[GPP_TRACK_MAX_TRACKS];                        /* column 12 of the row it last matched */
    double box[GPP_TRACK_FIELDS][GPP_TRACK_MAX_TRACKS];       /* field-major: box[f][slot] */
    int32_t next_id;                                          /* the id the next birth gets */
    int32_t frames;                                           /* frame steps so far */
    int32_t dropped;                                          /* births that found no free slot */
    int32_t reserved;
} gpp_track_state;
typedef struct gpp_track_params {
    int32_t metric;                      /* GPP_TRACK_BEV | GPP_TRACK_3D | GPP_TRACK_DIST */
    int32_t max_age;
    int32_t smooth;
    int32_t reserved;                    /* must be 0 */
    double threshold;
    double gain_a, gain_b, gain_c;       /* position, velocity, dimensions */
    double birth_score;
} gpp_track_params;
int gpp_track_state_bytes(size_t* bytes);                     /* sizeof(gpp_track_state) */
int gpp_track_workspace_bytes(int S, size_t* bytes);
int gpp_track_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                  const gpp_track_params* params, float* rows_out, int32_t* track_ids, int32_t* track_hits,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tracking with an OPTIMAL one-to-one assignment per frame (csrc/track.hip, the same kernel with another step 4; DESIGN.md section 4.32 is
 * the specification, utils/track.py with 'assign': 'optimal' the host form).  The signature, the structs, the state's layout, the
 * workspace, every error and the N * D == 0 / S == 0 behaviour are gpp_track_f64's; so are the steps 1 - 3 and 5 - 7 of the frame step,
 * operation for operation, and the candidates are the same pairs.  gpp_track_params has no field for the choice (reserved != 0 is refused
 * by both): the entry point is the choice.  Step 4 is:
 *
 *   matrix      square, int32, of side n = max(T, R): the T occupied slots in ascending slot order are its rows, the R live, non-blind rows
 *               of the frame in ascending row order its columns.  n == 0: nothing to do.
 *   cells       with S = 2^20 (GPP_MOT_SCALE_BITS).  GPP_TRACK_DIST: t2 = threshold * threshold, r = q / t2, x = r * 2^20 (three separate
 *               float64 operations); the cell is min(floor(x), S - 1).  GPP_TRACK_BEV / GPP_TRACK_3D: k = floor(min(o * 2^20, 2^20)); the
 *               cell is min(S - k, S - 1).  A pair that is no candidate has S, and so has every padding cell: a candidate's cell lies in
 *               [0, S - 1], so taking it is always better than leaving both sides alone.
 *   objective   the minimum total of the n assigned cells, that is the largest sum of (S - cell) over the candidates taken.  This is NOT
 *               gpp_mot_assign's GPP_MOT_BIG form ("most pairs first"): an unmatched pair costs what a pair at the threshold costs, and a
 *               near pair is given up for two farther ones only when those two together cost less than the near pair and one miss.
 *   assignment  gpp_mot_assign's paragraph "assignment" below, word for word: the rows in order, one shortest augmenting path each, int64
 *               potentials that start at zero, ties to the first column (csrc/mot_assign.h, gpp_mot::assign_rows, run by one wavefront on
 *               the matrix in LDS).  Everything behind the cells is integer: the three forms are equal with ==, ties included.
 *   pairs       slot i and row j are matched iff column j is assigned to row i and (i, j) is a candidate (its cell is below S).
 *
 *   workspace   gpp_track_workspace_bytes(S) bytes as gpp_track_f64 takes them (one buffer serves both entry points); only seq_start's copy
 *               is used: the matrix lies in LDS, 64 KiB at n = 128 beside the 81 KiB of the rest.
 * ---------------------------------------------------------------------------------------- */
int gpp_track_optimal_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                          const gpp_track_params* params, float* rows_out, int32_t* track_ids, int32_t* track_hits,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tracking with EGO-MOTION compensation (csrc/track.hip, either kernel with a step 1b; DESIGN.md section 4.33 is the specification,
 * utils/track.py with `ego` the host form, utils/oxts.py makes the records from KITTI's oxts and calib files).  The camera of a driving
 * car moves: without this step a parked car leaves its prediction by the ego displacement of every frame.  The state's layout,
 * gpp_track_params, every error and the N * D == 0 / S == 0 behaviour are gpp_track_f64's; steps 2 - 8 are those of the chosen
 * assignment, operation for operation.
 *
 *   ego         (N, GPP_TRACK_EGO_FIELDS) float64 on the HOST, like seq_start: one record per frame of the call -- R row-major (9),
 *               t (3), dyaw (1), then three words that must be 0.  A point p in the camera coordinates of the frame BEFORE f in its
 *               sequence lies at R p + t in the camera coordinates of frame f.  A call may continue an earlier one: the record of a
 *               call's first frame relates to the last frame of the call before.  With an empty tracker a record has no effect.
 *   assign      GPP_TRACK_ASSIGN_GREEDY: step 4 of gpp_track_f64; GPP_TRACK_ASSIGN_OPTIMAL: step 4 of gpp_track_optimal_f64.
 *   frame step  step 1 becomes, for every occupied slot, in this order:
 *     1a predict   as gpp_track_f64: x += vx, y += vy, z += vz.
 *     1b ego       x' = ((R00 x + R01 y) + R02 z) + t0, y' and z' likewise from rows 1 and 2 of R, all three from the old x y z;
 *                  vx' = (R00 vx + R01 vy) + R02 vz, vy' and vz' likewise; r_y' = wrap(r_y + dyaw), the wrap of gpp_pose_f32.  Every
 *                  multiply and every add is one separate float64 operation in exactly this association.  h w l are untouched.
 *               Velocity thereby means the object's own displacement per frame in the current camera's axes: a parked car has v = 0.
 *               dyaw is GIVEN, not derived from R: the host form derives it as atan2(R02 - R20, R00 + R22), which is exact for a
 *               rotation about the camera's Y axis and the nearest yaw otherwise.  Pitch and roll move positions and velocities through
 *               the full R; r_y only takes the yaw.  Smoothed rows are in the frame's own camera coordinates, as before.
 *   workspace   gpp_track_ego_workspace_bytes(S, N) bytes on the device, 8-byte aligned: gpp_track_workspace_bytes(S) and behind them
 *               the records' copy, 128 bytes per frame of the call (the entry point copies `ego` there as it copies seq_start).
 *
 *   GPP_ERR_BAD_ARG, nothing launched and nothing written, beyond gpp_track_f64's: a null `ego` when N > 0; an unknown `assign`; a
 *   non-finite value among the 13 words of the record of any frame inside a sequence; a padding word that is not 0.  The records are
 *   checked on the host, so that no NaN enters a slot through them.  Frames outside every sequence are neither checked nor read.
 * ---------------------------------------------------------------------------------------- */
#define GPP_TRACK_EGO_FIELDS 16
#define GPP_TRACK_ASSIGN_GREEDY 0
#define GPP_TRACK_ASSIGN_OPTIMAL 1
int gpp_track_ego_workspace_bytes(int S, int N, size_t* bytes);
int gpp_track_ego_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                      const gpp_track_params* params, const double* ego, int assign, float* rows_out, int32_t* track_ids,
                      int32_t* track_hits, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tracking with a KALMAN FILTER on the ground plane (csrc/track.hip, either kernel of either assignment with a covariance per slot;
 * DESIGN.md section 4.34 is the specification -- every expression below is written out there, fully parenthesised --, utils/track.py with
 * 'filter': 'kalman' the host form).  Every carried cuboid keeps the 4 x 4 covariance of (x, z, vx, vz); a row's measurement noise grows
 * with its range along the viewing ray and stays small across it; a matched pair is updated with the Kalman gain of the two, and the
 * fourth metric GPP_TRACK_MAHA gates and ranks by the squared Mahalanobis distance.  The state's layout, gpp_track_params, every error
 * and the N * D == 0 / S == 0 behaviour are gpp_track_ego_f64's; the three entry points above go on refusing GPP_TRACK_MAHA.
 *
 *   cov_in, cov_out (S, gpp_track_cov) on the device, 8-byte aligned: per slot the upper triangle of the symmetric covariance as three
 *               blocks, field-major like `box` -- A (position-position) Axx Axz Azz, B (position-velocity, a general 2 x 2: B[p][v])
 *               Bxx Bxz Bzx Bzz, C (velocity-velocity) Cxx Cxz Czz.  All zero for a free slot.  cov_out == cov_in is allowed, otherwise
 *               the two do not overlap.
 *   kf          radial0 + radial1 rho and tangential0 + tangential1 rho are the standard deviations of a row at range rho along and
 *               across its viewing ray (metres, metres per metre); q_pos, q_vel the process variances per frame step; birth_speed the
 *               standard deviation of a born track's velocity per component.
 *   ego         as gpp_track_ego_f64 takes it, or null: no records, no step 1b.
 *   frame step  that of gpp_track_ego_f64 (without 1b for a null `ego`) with:
 *     row noise    once per live, non-blind row: rho = sqrt(x x + z z), u = (x, z) / rho (u = (0, 1) for rho == 0),
 *                  R = st^2 I + (sr^2 - st^2) u u^T with sr = radial0 + radial1 rho, st = tangential0 + tangential1 rho.
 *     1 predict    the mean as before; A += B + B^T + C + q_pos I, B += C, C += q_vel I, all from the old values.
 *     1b ego       the mean as before; A, B and C each go to Rg X Rg^T with Rg = [[R00, R02], [R20, R22]] of the record.  What pitch and
 *                  roll mix in from y is left out.
 *     3 candidates GPP_TRACK_MAHA: S = A + R, det = Sxx Szz - Sxz Sxz, m = r^T S^-1 r for r = row - predicted in (x, z); a candidate
 *                  iff det > 0 and m < threshold * threshold (threshold: standard deviations, finite and > 0); the smaller m is
 *                  better; the key and the optimal form's cell are GPP_TRACK_DIST's with m in the place of q.  The other three metrics
 *                  gate and rank as before.
 *     5 update     S and det of the matched pair as above.  det > 0: K = [A; B^T] S^-1, (x, z, vx, vz) += K r, P -= K [A B] (upper
 *                  triangle).  Otherwise (only under BEV / 3D / DIST, from a caller's covariance): x z vx vz take the fixed gains and
 *                  the covariance is set as at a birth from the matched row.  y, vy, h w l and r_y keep their fixed gains always.
 *     6 deaths     the freed slot's covariance is zeroed.
 *     7 births     A = R of the row, B = 0, C = birth_speed^2 I.
 *   workspace   gpp_track_ego_workspace_bytes(S, N) bytes, with or without records.
 *
 *   GPP_ERR_BAD_ARG, nothing launched and nothing written, beyond gpp_track_ego_f64's (whose null `ego` is no error here): a null `kf`;
 *   radial0, tangential0 or birth_speed not finite and > 0; radial1, tangential1, q_pos or q_vel not finite and >= 0; kf->reserved != 0;
 *   a GPP_TRACK_MAHA threshold that is not finite and > 0; a null cov_in or cov_out when S > 0.  cov_in or cov_out not 8-byte aligned:
 *   GPP_ERR_ALIGN.  N * D == 0 (S > 0): state_in is copied to state_out and cov_in to cov_out.
 * ---------------------------------------------------------------------------------------- */
#define GPP_TRACK_MAHA 3
#define GPP_TRACK_COV_FIELDS 10          /* Axx Axz Azz  Bxx Bxz Bzx Bzz  Cxx Cxz Czz */
typedef struct gpp_track_cov {
    double p[GPP_TRACK_COV_FIELDS][GPP_TRACK_MAX_TRACKS];    /* field-major: p[f][slot] */
} gpp_track_cov;
typedef struct gpp_track_kf_params {
    double radial0, radial1;             /* sigma along the viewing ray: radial0 + radial1 * range */
    double tangential0, tangential1;     /* sigma across it */
    double q_pos, q_vel;                 /* process variances per frame step */
    double birth_speed;                  /* sigma of a born track's velocity */
    int64_t reserved;                    /* must be 0 */
} gpp_track_kf_params;
int gpp_track_cov_bytes(size_t* bytes);                       /* sizeof(gpp_track_cov) */
int gpp_track_kf_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                     const void* cov_in, void* cov_out, const gpp_track_params* params, const gpp_track_kf_params* kf,
                     const double* ego /* may be null */, int assign, float* rows_out, int32_t* track_ids, int32_t* track_hits,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * SMOOTHING finished tracks offline: a backward Rauch-Tung-Striebel pass over the forward filter above, and the filling of short gaps
 * (csrc/track_smooth.hip; DESIGN.md section 4.35 is the specification -- every expression is written out there, fully parenthesised --,
 * utils/track_smooth.py the host form and the maker of the index).  The tracker writes filtered positions: the cuboid at frame k knows
 * nothing of the frames behind it.  A finished run is in hand as a whole; this stage runs the filter of gpp_track_kf_f64 forward over
 * every SEGMENT of an identity -- (x, z, vx, vz), the same row noise, predict, ego step, update and birth -- and then backward, and
 * gives every detected row of the segment its smoothed x, z and alpha, every frame the detector missed inside the segment a FILL row,
 * and both the position block of the smoothed covariance.  Two launches, plain float64, every operation separate.
 *
 *   rows_in, rows_out (N, D, GPP_POSE_COLS) float32, device: the RAW rows of a finished run (not `smooth`ed ones).  rows_out == rows_in is
 *               allowed; otherwise the two do not overlap and rows_in is copied first.  D <= GPP_KITTI_MAX_DETECTIONS.
 *   the index   HOST arrays, like seq_start and the ego records; checked here before any launch and copied behind the workspace.
 *     seg_start (n_seg + 1) int64: segment s owns the cells [seg_start[s], seg_start[s + 1]); seg_start[0] == 0, ascending, every segment
 *               has at least one cell, seg_start[n_seg] == cells.
 *     seg_frame (n_seg) int32: the frame of the segment's first cell; cell c of the segment is frame seg_frame[s] + c, which is < N.
 *     cell_row  (cells) int32: the flat row index frame * D + d of the cell's detection, which lies in the cell's own frame, or -1 for a
 *               GAP: the track was alive and no row carried its id.  A segment's first and last cell are detections; no row has two cells.
 *               The order of the segments is free and no output depends on it (the entry point orders them by length for its lanes).
 *   kf          the noise of gpp_track_kf_f64.
 *   ego         (N, GPP_TRACK_EGO_FIELDS) float64 on the host, or null: as gpp_track_kf_f64 takes it; record f carries frame f - 1 to f.
 *   the rule    per segment, cell 0 is a birth from its row: mean (x, z, 0, 0), A = R of the row, B = 0, C = birth_speed^2 I.  Every later
 *               cell: predict; with records the ego step (the covariance as above; the mean by the ground part only, x' = (g00 x + g01 z)
 *               + t0, z' = (g10 x + g11 z) + t2, v through Rg -- what pitch and roll mix in from y is left out); at a detection the
 *               update, or, when det is not > 0, a restart as at a birth from the row.  Backward from the last cell, whose smoothed state
 *               is its filtered one: J = P_f(c) Phi^T P_p(c + 1)^-1 with Phi = blockdiag(Rg, Rg) F, the inverse by 2 x 2 blocks (A^-1, the
 *               Schur complement C - B^T A^-1 B and its inverse); J = 0 when either determinant is not > 0 or the step is a restart;
 *               x_s(c) = x_f(c) + J (x_s(c + 1) - x_p(c + 1)), P_s(c) = P_f(c) + J (P_s(c + 1) - P_p(c + 1)) J^T.
 *   rows_out    a detected row of a segment of two or more cells: columns 19 and 21 = x_s, z_s rounded to float32 once, column 25 =
 *               wrap(r_y - atan2(x_s, z_s)) with the row's own r_y.  Every other column and every other row is a bit copy.
 *   row_cov     (N, D, 3) float64, device, may be null: Axx Axz Azz of P_s for those rows, zeros everywhere else.
 *   fill_rows   (fills, GPP_POSE_COLS) float32, device, fills = the number of gaps: one row per gap in cell order.  With a and b the
 *               detected neighbours before and behind, at cells c0 < c < c1 of the segment, and w = (c - c0) / (c1 - c0): columns 19 21 25
 *               as above, with the fill's own r_y; column 32 (r_y) = wrap(a + w d), d = wrap(b - a) brought into [-pi/2, pi/2) by a half
 *               turn; the columns 13 14 33 34 35 hold codes and padding and come from a; every other column is a + w (b - a) in float64,
 *               rounded once -- y among them, which is NOT ego-compensated.  May be null when there is no gap.
 *   fill_cov    (fills, 3) float64, device, may be null: Axx Axz Azz of P_s per fill.
 *   workspace   gpp_track_smooth_workspace_bytes(N, n_seg, cells) bytes on the device, 8-byte aligned: 28 float64 per cell in blocks of
 *               64 segments, five per cell for the smoothed table, and the copies of the index and the records.
 *
 *   GPP_ERR_BAD_ARG, nothing launched and nothing written: a negative N, D, n_seg or cells; D > GPP_KITTI_MAX_DETECTIONS; N * D beyond
 *   2^31 - 1; a null kf, seg_start, or seg_frame / cell_row / workspace / fill_rows where they are needed, or rows when N * D > 0; the noise
 *   refusals of gpp_track_kf_f64; offsets that do not ascend as stated; a frame or a row index out of range, a row outside its cell's
 *   frame or in two cells; a segment whose first or last cell is a gap; cells > 0 with N * D == 0; a non-finite word among the first 13 of
 *   any record, or a padding word that is not 0.  GPP_ERR_ALIGN: rows, row_cov, fill_rows, fill_cov not 4 / 8-byte aligned, the workspace
 *   not 8-byte aligned.  GPP_ERR_WORKSPACE.  cells == 0 or N * D == 0: rows_in is copied to rows_out, row_cov is zeroed, nothing is launched.
 * ---------------------------------------------------------------------------------------- */
int gpp_track_smooth_workspace_bytes(int N, int n_seg, long long cells, size_t* bytes);
int gpp_track_smooth_f64(const float* rows_in, int N, int D, const int64_t* seg_start, const int32_t* seg_frame, const int32_t* cell_row,
                         int n_seg, const gpp_track_kf_params* kf, const double* ego /* may be null */, float* rows_out,
                         double* row_cov /* may be null */, float* fill_rows, double* fill_cov /* may be null */, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CLEAR-MOT scoring of tracks on the device (csrc/mot_eval.hip; DESIGN.md section 4.29 is the specification, a restatement of the KITTI
 * tracking devkit's CLEAR-MOT -- parity with the devkit itself is UNPINNED; utils/mot_eval.py is the host form): per frame the OPTIMAL
 * one-to-one assignment of the tracker's rows to the labels (the Hungarian method, shortest augmenting paths, exact integers), then per
 * sequence the identity switches, fragmentations and mostly-tracked / mostly-lost shares.  Two launches.
 *
 *   overlaps (N, 4, D, A) float64, labels (N, A, GPP_KITTI_LABEL_COLS) float64, label_counts (N) int32 (clamped to [0, A]), rows
 *   (N, D, GPP_POSE_COLS) float32, device: exactly what gpp_kitti_overlaps_f64 took and wrote.  ids (N, D) int32, device: the tracker's id
 *   of every row, in the layout gpp_track_f64 writes.  A row is a ROW of the assignment iff its column 14 is >= 0 and its id is >= 0.
 *
 * gpp_mot_assign: one frame per workgroup of one wavefront; the frame's cost matrix lies in LDS.
 *   status      of label a < count, from its type code (column 0): a Car (0) COUNTS, unless occlusion (column 2) > max_occlusion or
 *               truncation (column 1) > max_truncation or |y2 - y1| (columns 7, 5) < min_height: then it is IGNORED; a Van (1) is IGNORED;
 *               DontCare (2) is a region only; anything else is not in play.  The labels in play are the counting and the ignored ones.
 *   matrix      square, of side n = max(G, T): G labels in play in ascending label order are its rows, T rows in ascending row order its
 *               columns.  With o the overlap of plane `metric` (0 image, 1 BEV, 2 3-D): the pair is admissible iff o >= min_overlap (not
 *               strict; float64; false for NaN); k = floor(min(o * 2^20, 2^20)); the cell is 2^20 - k if admissible, GPP_MOT_BIG otherwise
 *               and in every padding cell.  n * 2^20 < GPP_MOT_BIG: the minimum total cost is "most admissible pairs, then the largest sum
 *               of k".
 *   assignment  the matrix's rows i = 0 .. n - 1 in order, each by one shortest augmenting path over int64 potentials u (rows), v
 *               (columns), all zero at the start.  Per row: minv = infinity, no column used, i0 = i.  Repeat: for every unused column j,
 *               cur = cell(i0, j) - u[i0] - v[j]; if cur < minv[j] then minv[j] = cur and way[j] = the column the step came from; delta =
 *               the smallest minv of the unused columns, j1 = the FIRST column that has it; u += delta on row i and on the row of every
 *               used column, v -= delta on every used column, minv -= delta on every unused one; j1 becomes used; if j1 holds a row,
 *               i0 = that row and repeat, otherwise the rows are handed back along way, j1 first, and row i takes the last column.
 *   match       (N, A) int32: the row index d that label a is paired with, -1 for none.  A pair whose cell is GPP_MOT_BIG is no pair.
 *   label_outcome (N, A) int32: 0 not in play, 1 counting and paired (a true positive), 2 counting and unpaired (a false negative),
 *               3 ignored and paired, 4 ignored and unpaired.
 *   row_outcome (N, D) int32: 0 no row, 1 paired with a counting label, 2 paired with an ignored label (neither true nor false positive),
 *               3 unpaired: a false positive, 4 unpaired and |y2 - y1| (columns 29, 27) < min_height, 5 unpaired and plane 3 of the overlaps
 *               (intersection over the row's area) with some DontCare label of the frame is > 0.5.
 *   frame_counts (N, GPP_MOT_FRAME_COUNTS) int64: true positives, false positives, false negatives, counting labels, the sum of k over
 *               the true positives, the assignment's total cost (all n cells), G, T.
 *   GPP_ERR_BAD_ARG, nothing launched: a null pointer that the sizes make necessary (A == 0: labels, label_counts, match, label_outcome and
 *   overlaps may be null; D == 0: rows, ids, row_outcome and overlaps may be null), a negative size, a metric other than 0 1 2, min_overlap
 *   outside [0, 1] or NaN, a NaN limit, reserved != 0.  D or A > 128: GPP_ERR_UNSUPPORTED.  N == 0: GPP_OK, nothing launched.  D == 0 is
 *   legal: every counting label is a false negative.  A == 0 is legal: every row that is high enough is a false positive.
 *
 * gpp_mot_clear: one workgroup per sequence, which walks its frames in order.
 *   seq_start   (S + 1) int32 on the HOST, as gpp_track_f64 takes it.
 *   traj        (N, A) int32, device: the trajectory of label a -- the index of its track_id among the sequence's track_ids, compacted by
 *               the host to [0, max_traj); a trajectory appears at most once per frame.  Read only where the label counts.
 *   per trajectory, over the frames in which it counts: counting += 1; paired: matched += 1, and if it was paired before: a SWITCH when
 *               the row's id differs from the id at its last paired frame, a FRAGMENTATION when its previous counting frame was unpaired.
 *   traj_table  (S, max_traj, GPP_MOT_TRAJ_COLS) int32: counting frames, matched frames, switches, fragmentations.
 *   seq_counts  (S, GPP_MOT_SEQ_COUNTS) int64: the sums of frame_counts' first six columns over the sequence's frames, then switches,
 *               fragmentations, mostly tracked (5 matched >= 4 counting), partly tracked, mostly lost (5 matched < counting), trajectories
 *               with a counting frame, frames, and three zeros.  Integer sums: the result does not depend on the order.
 *   max_traj <= GPP_MOT_MAX_TRAJECTORIES: the state of a sequence's trajectories lies in LDS (21 KiB at the cap); beyond:
 *   GPP_ERR_UNSUPPORTED, as D or A > 128.  workspace: gpp_mot_clear_workspace_bytes(S) bytes on the device, 4-byte aligned (seq_start's
 *   copy); short: GPP_ERR_WORKSPACE.  Null pointer, negative size, a seq_start that is not monotone inside [0, N]: GPP_ERR_BAD_ARG,
 *   nothing launched.  S == 0: GPP_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
#define GPP_MOT_SCALE_BITS 20
#define GPP_MOT_BIG (1 << 28)
#define GPP_MOT_MAX_TRAJECTORIES 1024
#define GPP_MOT_FRAME_COUNTS 8
#define GPP_MOT_SEQ_COUNTS 16
#define GPP_MOT_TRAJ_COLS 4
typedef struct gpp_mot_params {
    int32_t metric;                      /* the overlaps' plane: 0 image, 1 BEV, 2 3-D */
    int32_t reserved;                    /* must be 0 */
    double min_overlap;                  /* the devkit: 0.5 */
    double max_occlusion;                /* 2 */
    double max_truncation;               /* 0 */
    double min_height;                   /* 25 */
} gpp_mot_params;
int gpp_mot_assign(const double* overlaps, const double* labels, const int32_t* label_counts, const float* rows, const int32_t* ids,
                   int N, int D, int A, const gpp_mot_params* params, int32_t* match, int32_t* label_outcome, int32_t* row_outcome,
                   int64_t* frame_counts, void* stream);
int gpp_mot_clear_workspace_bytes(int S, size_t* bytes);
int gpp_mot_clear(const int32_t* match, const int32_t* label_outcome, const int32_t* traj, const int32_t* ids,
                  const int64_t* frame_counts, int N, int D, int A, const int32_t* seq_start, int S, int max_traj,
                  int64_t* seq_counts, int32_t* traj_table, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * HOTA scoring of tracks on the device (csrc/hota_eval.hip; DESIGN.md section 4.30 is the specification -- parity with TrackEval's hota.py
 * and its KITTI preprocessing is UNPINNED; utils/hota_eval.py is the host form): the alignment score of every (label trajectory, tracker
 * id) pair of a sequence, per frame the OPTIMAL assignment on costs that this score weighs (section 4.29's routine, csrc/mot_assign.h),
 * per sequence the detection, association and localisation integers at the GPP_HOTA_LEVELS thresholds j / 20.  Three launches, plain
 * launches in stream order.  Exact integers: every sum is an integer sum and does not depend on the order.
 *
 *   overlaps (N, 4, D, A) float64: gpp_kitti_overlaps_f64's.  label_outcome (N, A) and row_outcome (N, D) int32: gpp_mot_assign's, run
 *   with the call's metric and limits -- HOTA's preprocessing.  A label COUNTS iff its label_outcome is 1 or 2; a row is KEPT iff its
 *   row_outcome is 1 or 3; both in ascending index order.
 *   traj (N, A) int32: as gpp_mot_clear takes it -- a counting label's trajectory g in [0, n_gt) of its sequence.
 *   trk (N, D) int32: a kept row's tracker t in [0, n_trk) -- the index of its id among the ids of its sequence, ascending -- else -1.
 *   (A counting label or kept row whose index lies outside its range is treated as not counting / not kept.)
 *   frame_tab (N, GPP_HOTA_TAB_COLS) int32 on the HOST, one line per frame of the call: cell_base, n_gt, n_trk, vec_base of the frame's
 *   sequence.  Cell (g, t) of the sequence's pair table is cell_base + g n_trk + t; gc[g] is counter vec_base + g, tc[t] is counter
 *   vec_base + n_gt + t.  A chunk of frames is a slice of every per-frame array and of frame_tab: no offsets to add.
 *   metric: the overlaps' plane, 0 image, 1 BEV, 2 3-D.  q = floor(min(o 2^20, 2^20)), 0 for NaN and o <= 0: every (counting label, kept
 *   row) pair has one; there is no admissibility test.
 *
 * workspace: gpp_hota_workspace_bytes(cells, vecs, max_frames, S) bytes on the device, 16-byte aligned, ZEROED by the caller before the
 *   first gpp_hota_potential; cells and vecs are the totals over all sequences, max_frames the most frames of one call.  Its layout, which
 *   a test may read: P int64[cells] at byte 0; the alignment A int32[cells] at 8 cells; hist int32[cells][GPP_HOTA_HIST] at 12 cells
 *   rounded up to 16; the counters gc / tc int32[vecs] behind hist; behind them, rounded up to 16, room for the call's copy of frame_tab
 *   or seq_tab.
 *
 * gpp_hota_potential (pass 1): one frame per workgroup; q, the sums rs[a] = sum_d q and cs[d] = sum_a q in LDS.
 *   p = floor(q 2^20 / (rs[a] + cs[d] - q)) for q > 0; P[g, t] += p (64-bit integer atomics); gc[g] += 1 per counting label, tc[t] += 1
 *   per kept row (32-bit).  Call it for EVERY frame of a sequence before gpp_hota_match for any.
 * gpp_hota_match (pass 2): one frame per workgroup of one wavefront; the matrix in LDS.
 *   A[g, t] = floor(P 2^20 / ((gc[g] + tc[t]) 2^20 - P)) for P > 0, else 0 (written to the workspace for every pair a frame holds).
 *   matrix      square, of side n = max(G', T'): the counting labels are its rows, the kept rows its columns; a cell is
 *               2^20 - ((A[g, t] q) >> 20), every padding cell 2^20.  The assignment is gpp_mot_assign's, operation for operation.
 *   a real pair (a, d) of the assignment has jm = min(19, (20 q + 19) >> 20), the largest j with floor(j 2^20 / 20) <= q.  If jm >= 1:
 *               hota_match[a] = d, hist[g, t][jm] += 1 (32-bit atomics), and for j = 1 .. jm: TP_j += 1, SQ_j += q.
 *   hota_match  (N, A) int32: the row index, -1 for none.
 *   frame_hota  (N, GPP_HOTA_FRAME_COLS) int64: TP_1 .. TP_19, SQ_1 .. SQ_19, G', T'.
 * gpp_hota_reduce: one thread per table cell, grid (blocks, S); per wavefront one 64-bit integer atomic per quantity and threshold.
 *   seq_tab     (S, GPP_HOTA_SEQ_TAB_COLS) int32 on the HOST: cell_base, n_gt, n_trk, vec_base, first frame, one past the last frame.
 *   mc_j[g, t] = sum over m >= j of hist[g, t][m]; over the cells with mc > 0: ASS_j += floor(mc^2 2^20 / (gc + tc - mc)),
 *               ASSRE_j += floor(mc^2 2^20 / gc), ASSPR_j += floor(mc^2 2^20 / tc).  TP_j, SQ_j: the sums of frame_hota over the
 *               sequence's frames; FN_j = sum G' - TP_j, FP_j = sum T' - TP_j.
 *   seq_hota    (S, GPP_HOTA_LEVELS, GPP_HOTA_SEQ_COLS) int64, ZEROED by the caller: TP, FN, FP, SQ, ASS, ASSRE, ASSPR, 0.
 *   At most 2^20 frames per sequence keep everything below 2^63 (the caller's to ensure: utils/hota_eval.py raises).
 *
 *   GPP_ERR_BAD_ARG, nothing launched: a null pointer that the sizes make necessary (A == 0: label_outcome, traj, hota_match and overlaps
 *   may be null; D == 0: row_outcome, trk and overlaps), a negative size, a metric other than 0 1 2, a table line with a negative entry,
 *   with a base below the line before it, or whose cells or counters leave [0, cells) / [0, vecs); a seq_tab whose frame ranges are not
 *   monotone inside [0, N].  D or A > 128, cells or vecs >= 2^31, S > 65535: GPP_ERR_UNSUPPORTED.  A workspace that is not 16-byte
 *   aligned: GPP_ERR_ALIGN; too short: GPP_ERR_WORKSPACE.  N == 0 (potential, match) or S == 0 (reduce): GPP_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
#define GPP_HOTA_LEVELS 19
#define GPP_HOTA_HIST 20
#define GPP_HOTA_FRAME_COLS 40
#define GPP_HOTA_SEQ_COLS 8
#define GPP_HOTA_TAB_COLS 4
#define GPP_HOTA_SEQ_TAB_COLS 6
int gpp_hota_workspace_bytes(long long cells, long long vecs, int max_frames, int S, size_t* bytes);
int gpp_hota_potential(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
                       const int32_t* trk, int N, int D, int A, int metric, const int32_t* frame_tab, long long cells, long long vecs,
                       void* workspace, size_t workspace_bytes, void* stream);
int gpp_hota_match(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
                   const int32_t* trk, int N, int D, int A, int metric, const int32_t* frame_tab, long long cells, long long vecs,
                   int32_t* hota_match, int64_t* frame_hota, void* workspace, size_t workspace_bytes, void* stream);
int gpp_hota_reduce(const int64_t* frame_hota, int N, const int32_t* seq_tab, int S, long long cells, long long vecs,
                    int64_t* seq_hota, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Identity scoring of tracks on the device -- IDF1, IDR, IDP (csrc/idf1_eval.hip; DESIGN.md section 4.31 is the specification -- parity
 * with TrackEval's identity.py is UNPINNED; utils/idf1_eval.py is the host form): per sequence the table C of how often every (label
 * trajectory, tracker id) pair overlaps by at least one half, then ONE optimal assignment per sequence of the trajectories to the tracker
 * ids on that table (section 4.29's rule in its rectangular form).  Two launches, plain launches in stream order.  Exact integers.
 *
 *   overlaps, label_outcome, row_outcome, traj, trk, frame_tab, seq_tab, metric, cells, vecs: exactly gpp_hota_potential's and
 *   gpp_hota_reduce's (above) -- the same arrays serve both scores.  frame_tab and seq_tab lie on the HOST.  q = floor(min(o 2^20, 2^20)),
 *   0 for NaN and o <= 0.
 *
 * workspace: gpp_idf1_workspace_bytes(cells, vecs, max_frames, S) bytes on the device, 16-byte aligned, ZEROED by the caller before the
 *   first gpp_idf1_count; max_frames is the most frames of one gpp_idf1_count call.  Its layout, which a test may read AND WRITE -- the
 *   assignment takes whatever table lies there, frames or no frames --: C int32[cells] at byte 0, cell (g, t) of a sequence at
 *   cell_base + g n_trk + t; the counters gc / tc int32[vecs] at 4 cells rounded up to 16, gc[g] at vec_base + g and tc[t] at
 *   vec_base + n_gt + t; behind them, rounded up to 16, room for the call's copy of frame_tab or seq_tab.
 *
 * gpp_idf1_count (pass 1): one frame per workgroup.  For every (counting label a, kept row d) of the frame with q(a, d) >= 2^19 -- the
 *   same as o >= 0.5: an overlap of exactly one half counts --, C[traj[a], trk[d]] += 1; there is no one-to-one rule inside a frame.
 *   gc[g] += 1 per counting label, tc[t] += 1 per kept row: section 4.30's counters.  32-bit integer atomics.  Call it for EVERY frame of
 *   a sequence before gpp_idf1_assign.
 * gpp_idf1_assign (pass 2): one sequence per workgroup of ONE wavefront; the table stays in device memory, the column state lies in LDS
 *   (24 bytes a column and 8 a row of the launch's largest sequence: 104 KiB at the limits).  Columns 4 and 5 of a seq_tab line are not read.
 *   matrix      G = n_gt rows by n = max(n_gt, n_trk) columns: the cell is 2^20 - C[g, t] for t < n_trk and 2^20 in every padding column.
 *   assignment  gpp_mot_assign's, operation for operation, for the rows i = 0 .. G - 1 in order: u = v = 0 at the start, int64
 *               potentials, strict < in the relaxation, the FIRST column on ties, the rows handed back along way.
 *   id_match    int32, vecs entries: id_match[vec_base + g] = the column of trajectory g if it is < n_trk and C[g, column] > 0, else -1
 *               (pairing a trajectory with an id it never met costs what leaving both alone costs).  The entries from vec_base + n_gt on
 *               are not written.
 *   seq_idf1    (S, GPP_IDF1_SEQ_COLS) int64: IDTP = the sum of C[g, id_match[g]], IDFN = sum gc - IDTP, IDFP = sum tc - IDTP, sum gc,
 *               sum tc, the assignment's total cost G 2^20 - IDTP, G, T.  Every entry is written.
 *   C <= 2^20 (at most 2^20 frames per sequence, the caller's to ensure: utils/hota_eval.tables raises) keeps every cell >= 0 and every
 *   potential below 2^33; the arg-min's packed key is minv << 13 | column.
 *
 *   GPP_ERR_BAD_ARG, nothing launched: a null pointer that the sizes make necessary (A == 0: label_outcome, traj and overlaps may be null;
 *   D == 0: row_outcome, trk and overlaps; no trajectory in any sequence: id_match), a negative size, a metric other than 0 1 2, a table
 *   line with a negative entry, with a base below the line before it, or whose cells or counters leave [0, cells) / [0, vecs).
 *   D or A > 128, cells or vecs >= 2^31, a sequence with n_gt > GPP_MOT_MAX_TRAJECTORIES or max(n_gt, n_trk) > GPP_IDF1_MAX_IDS:
 *   GPP_ERR_UNSUPPORTED.  A workspace that is not 16-byte aligned: GPP_ERR_ALIGN; too short: GPP_ERR_WORKSPACE.  N == 0 (count) or S == 0
 *   (assign): GPP_OK, nothing launched.  A sequence with n_gt == 0 or n_trk == 0: GPP_OK, IDTP 0, every id_match -1.
 * ---------------------------------------------------------------------------------------- */
#define GPP_IDF1_MAX_IDS 4096
#define GPP_IDF1_SEQ_COLS 8
int gpp_idf1_workspace_bytes(long long cells, long long vecs, int max_frames, int S, size_t* bytes);
int gpp_idf1_count(const double* overlaps, const int32_t* label_outcome, const int32_t* row_outcome, const int32_t* traj,
                   const int32_t* trk, int N, int D, int A, int metric, const int32_t* frame_tab, long long cells, long long vecs,
                   void* workspace, size_t workspace_bytes, void* stream);
int gpp_idf1_assign(const int32_t* seq_tab, int S, long long cells, long long vecs, int32_t* id_match, int64_t* seq_idf1,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * KITTI keypoint ("mod") labels on the device (csrc/label_prep.hip; DESIGN.md section 4.18 is the specification, utils/label_prep.py the
 * host form): what the reference's label_prep/create_mod_labels.m, computeBox3D.m and projectToImage.m make of a label_2 row and the
 * camera-2 matrix -- the 20 fields that bin/evaluate.py and KittiGenerator read.  Parity with MATLAB itself is UNPINNED.  One launch,
 * one thread per (image, label row), float64 with every operation separate.
 *
 *   labels (B, A, GPP_KITTI_LABEL_COLS) float64, label_counts (B) int32 (clamped to [0, A]), device: as gpp_kitti_overlaps_f64 takes
 *   them -- one upload serves both.
 *   P (B, 3, 4) float64, device: per image the camera-2 matrix at scale 1.
 *   trig (B, A, 2) float64, device: cos(r_y) and sin(r_y) of every row, computed on the HOST for the host form and the device form alike
 *   (device libm, glibc and MATLAB each round the last bit their own way).  The kernel is left with + - * /, minimum, maximum and
 *   compares: its result equals the NumPy form bit for bit.
 *
 *   per row     the corners 1..8 of computeBox3D.m:22-24, X = c x + s z + t_x, Y = y + t_y, Z = -s x + c z + t_z.  Any Z < 0.1: the row is
 *               DEMOTED.  Otherwise each corner is projected -- ((P_r0 X + P_r1 Y) + P_r2 Z) + P_r3 per row r, then u / w and v / w --,
 *               deg = (180 / pi) alpha, the orientation class is 0 for deg in [0, 90), 1 for [90, 180), 2 for [-90, 0), 3 for [-180, -90),
 *               the keypoints l m r t are the corners 3 2 1 6 | 2 1 4 5 | 4 3 2 7 | 1 4 3 8 of class 0 | 1 | 2 | 3 and the box is the
 *               minimum / maximum over the eight projected corners, unclipped.
 *               deg outside [-180, 180) (or NaN) is out of contract (the MATLAB script would reuse the previous object's variables): the
 *               row is demoted here; the host reader raises ValueError.
 *   mod (B, A, GPP_LABEL_MOD_COLS) float64:
 *     column    a valid row                                   a demoted row
 *      0        type code of the label                        2 (DontCare)
 *      1 -  3   truncation, occlusion, alpha                  -1, -1, -10
 *      4 -  7   the prepared box x1 y1 x2 y2                  the label's own box
 *      8 - 15   xl yl xm ym xr yr xt yt                       -10000
 *     16 - 18   h w l                                         h w l
 *     19        orientation class                             -1
 *     rows at or beyond the count: -1 in every column.
 *   boxes (B, A, 12) dims (B, A, 3) scores (B, A) float32, det_labels / orientations (B, A) int32: ALL five or NONE (null).  The layout
 *   gpp_detect_f32 leaves its outputs in, so that gpp_poll_f32 and gpp_pose_f32 read them in place (D = A).  Row a is a detection iff it
 *   is valid and bit `type code` of det_types is set: then the box (own_box != 0: the label's own 2-D box, own_box == 0: the prepared
 *   box), the keypoints and h w l, each double rounded to float32 once, score 1, label 0, its orientation class.  Every other row is
 *   the -1 padding of gpp_detect_f32.
 *
 *   Null pointer (or some but not all of the five), negative size: GPP_ERR_BAD_ARG, nothing launched.  B * A == 0: GPP_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
#define GPP_LABEL_MOD_COLS 20
int gpp_label_prep_f64(const double* labels, const int32_t* label_counts, const double* P, const double* trig, int B, int A,
                       unsigned det_types, int own_box, double* mod,
                       float* boxes, float* dims, float* scores, int32_t* det_labels, int32_t* orientations, void* stream);

/* ------------------------------------------------------------------------------------------
 * Plane-database distillation (csrc/plane_db.hip; DESIGN.md section 4.21 is the specification, utils/plane_db.py the host side): from a
 * pool of M candidate planes and the objects of a labelled dataset, the K planes that polling on that dataset loses least with.
 *
 * gpp_poll_costs_u16: the cost of serving object o with plane p alone, for every pair.  One workgroup per listed row, the pair arithmetic
 * of gpp_poll_f32 (csrc/poll_eval.h: the same float32 operations in the same order).
 *   boxes (B, D, 12), dims (B, D, 3), orient (B, D), P_inv (B, 4, 3), thr: exactly as gpp_poll_f32 takes them.
 *   planes (M, 4) float32, 16-byte aligned, shared by the batch; canonicalised into the workspace as gpp_poll_f32 does.
 *   row_index (O) int32: the flat rows b * D + d to evaluate, in table order; NULL: all B * D rows in order, and O must be B * D.
 *   table: uint16, 16-byte aligned, `pitch` values per row with pitch >= M and pitch % 8 == 0.  Listed row i fills the columns [0, M) of
 *   table row row_offset + i (row_offset >= 0: a dataset is filled chunk by chunk); the columns [M, pitch) are left untouched.
 *   per pair, with zc, votes and res as polling computes them (votes of the six segments, res their residual SUM in metres):
 *       invalid, if zc < 0.0f is true or res < FLT_MAX is false (a NaN residual):       key = GPP_PLANE_COST_INVALID
 *       otherwise   s = res * 1024.0f,  q = (s < 8191.0f) ? (int)s : 8191,              key = (6 - (int)votes) * 8192 + q   (<= 57343)
 *   the order in which polling itself ranks the planes of one object -- votes first, then the residual -- quantised to 1/1024 m.
 *   A row whose orient is negative (the -1 padding of gpp_label_prep_f64), or a list entry outside [0, B * D), is
 *   GPP_PLANE_COST_INVALID throughout.
 *   workspace: gpp_poll_costs_workspace_bytes() bytes, 16-byte aligned (the canonical planes).
 *   Null pointer, negative size, pitch < M or pitch % 8 != 0, O != B * D without a list: GPP_ERR_BAD_ARG; planes, table or workspace not
 *   16-byte aligned: GPP_ERR_ALIGN; a short workspace: GPP_ERR_WORKSPACE; nothing is launched in any of these cases.
 *   O * M == 0: GPP_OK, nothing launched.
 *
 * gpp_plane_select: greedy facility location on the table, in exact integers.
 *   table, pitch: as above (16-byte aligned, pitch >= M, pitch % 8 == 0), O >= 1 rows, M >= 1 planes, 1 <= K <= M picks.
 *   state       best[o] = 65535 for every row, trace[0] = 65535 * O.
 *   pick k      gain[p] = sum over o of max(0, best[o] - table[o][p]);  p* = the FIRST index of the largest gain.
 *               gain[p*] == 0: the run stops -- count stays k, chosen[k..K) = -1, trace[k+1..K] repeat trace[k].
 *               otherwise chosen[k] = p*, best[o] = min(best[o], table[o][p*]), trace[k + 1] = trace[k] - gain[p*], count = k + 1.
 *   The pick order is the result: the first K' entries of a run with K >= K' are the run with K'.  A plane is never picked twice (its
 *   gain is 0 once it is in), and of two equal columns only the first can be picked.
 *   chosen (K) int32, trace (K + 1) uint64 (8-byte aligned), best (O) uint16, count (1) int32: device, all written.
 *   workspace: gpp_plane_select_workspace_bytes() bytes, 16-byte aligned (gain (M) uint64, then the done flag).
 *   2 K + 1 plain launches in stream order: per pick one launch of ceil(O / 256) x ceil(M / 512) workgroups that adds the gains (16-byte
 *   loads of 8 planes of a row, 32-bit partial sums over a slab of 256 rows, 64-bit atomic adds: integer sums do not depend on the order)
 *   and one single-workgroup launch that picks, lowers `best` and clears the gains.  Once the run has stopped the remaining launches
 *   return at once.  Nothing is read back: the caller fetches `count` when the stream has finished.
 *   K > M, K < 1, O < 1, M < 1, a bad pitch or a null pointer: GPP_ERR_BAD_ARG; alignment: GPP_ERR_ALIGN; a short workspace:
 *   GPP_ERR_WORKSPACE; nothing is launched in any of these cases.
 * ---------------------------------------------------------------------------------------- */
#define GPP_PLANE_COST_INVALID 65535
int gpp_poll_costs_workspace_bytes(int M, size_t* bytes);
int gpp_poll_costs_u16(const float* boxes, const float* dims, const int32_t* orient, const float* P_inv, const float* planes,
                       int B, int D, int M, float thr, const int32_t* row_index, int O, uint16_t* table, int64_t pitch,
                       int64_t row_offset, void* workspace, size_t workspace_bytes, void* stream);
int gpp_plane_select_workspace_bytes(int M, size_t* bytes);
int gpp_plane_select(const uint16_t* table, int O, int M, int64_t pitch, int K, int32_t* chosen, uint64_t* trace,
                     uint16_t* best, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The same distillation for the location error that polling leaves (csrc/plane_db.hip, csrc/pose_eval.h; DESIGN.md section 4.23 is the
 * specification, utils/plane_db.py the host side and the NumPy form).  Opt-in: nothing above changes.
 *
 * gpp_pose_costs_u16: two tables from one evaluation of every pair, both uint16, (O, pitch), laid out as the table above.
 *   keys[o][p]  exactly what gpp_poll_costs_u16 writes for the same call.
 *   errs[o][p]  the distance between the location that pose recovery gives object o when polling has plane p alone, and the label's.
 *   want (B, D, 3) float32: the labels' locations (label columns 11:14, rounded to float32 once on the host), indexed like dims.
 *   With X[0..3] = X_l, X_m, X_r, X_t of the pair, o = orient, w = dims[1], float32, every operation separate, norm3 and cross3 as in
 *   csrc/poll_eval.h (norm3(a) = sqrt((a.x a.x + a.y a.y) + a.z a.z)):
 *       X_s = (o == 0 || o == 3) ? X_l : X_r
 *       h = norm3(X_t - X_m),  e = norm3(X_s - X_m)
 *       y = (X_m - X_t) / h                        component by component
 *       x = (sx * (X_m - X_s)) / e                 sx = +1, +1, -1, -1 for o = 0..3
 *       z = cross3(x, y)
 *       loc = (X_m + X_s) / 2 + ((sz * z) * w) / 2                sz = +1, -1, +1, -1 for o = 0..3
 *       dist = norm3(loc - want),  s = dist * 256.0f,  q = (s < 65534.0f) ? (int)s : 65534     (a NaN or infinite s: 65534)
 *       errs = GPP_PLANE_COST_INVALID exactly where keys is, else q: 1/256 m per quantum, saturating just below 256 m.
 *   Every other argument, the checks, the alignment (keys and errs both), the workspace (gpp_poll_costs_workspace_bytes), padding rows,
 *   list entries outside the batch (both tables GPP_PLANE_COST_INVALID) and the untouched pad columns: exactly as gpp_poll_costs_u16.
 *
 * gpp_plane_select_polled: a greedy selection on the two tables for the error of the plane that polling itself would pick.
 *   state       best[o] = cur[o] = 65535 for every row: the smallest key among the picks so far and the error of the plane that holds it;
 *               trace[0] = 65535 * O.
 *   pick k      gain[p] = sum over o with keys[o][p] < best[o] of (cur[o] - errs[o][p]): a signed 64-bit sum, its terms may be negative.
 *               p* = the FIRST index of the largest gain.  gain[p*] <= 0: the run stops -- count stays k, chosen[k..K) = -1,
 *               trace[k+1..K] repeat trace[k].  Otherwise chosen[k] = p*; for the rows with keys[o][p*] < best[o]: best[o] = keys[o][p*],
 *               cur[o] = errs[o][p*]; trace[k + 1] = trace[k] - gain[p*], count = k + 1.
 *   The inequality is strict: the incumbent stands earlier in the written database, and polling gives equal candidates to the lower index.
 *   trace[j] is the sum of cur after the first j picks and falls strictly up to count; no plane is picked twice (a chosen plane has no
 *   strictly lower key: its gain is 0); the first K' picks of a longer run are the run with K'; the first pick is the best single plane.
 *   Beyond the first pick this is a greedy heuristic on an objective that is not monotone: a pick can raise some rows' errors, and a
 *   plane that would lower the sum only together with another one is never found.
 *   chosen (K) int32, trace (K + 1) uint64 (8-byte aligned), best (O), cur (O) uint16, count (1) int32: device, all written.
 *   workspace: gpp_plane_select_polled_workspace_bytes() bytes, 16-byte aligned (gain (M) int64, then the done flag).
 *   2 K + 1 plain launches in stream order, as gpp_plane_select: the gain launch reads 8 planes of a row from each table with two 16-byte
 *   loads, keeps signed 32-bit partial sums over a slab of 256 rows (at most 256 x 65535 < 2^24 in magnitude), adds them in LDS and then
 *   into the 64-bit gains with integer atomics (two's-complement addition does not depend on the order); the single-workgroup launch
 *   takes the lexicographic (signed gain, -index) maximum, updates best and cur along the column and clears the gains.  Pad columns are
 *   read and never counted.  Error codes as gpp_plane_select (keys and errs both checked); nothing is launched on a bad argument.
 * ---------------------------------------------------------------------------------------- */
int gpp_pose_costs_u16(const float* boxes, const float* dims, const int32_t* orient, const float* P_inv, const float* want,
                       const float* planes, int B, int D, int M, float thr, const int32_t* row_index, int O, uint16_t* keys,
                       uint16_t* errs, int64_t pitch, int64_t row_offset, void* workspace, size_t workspace_bytes, void* stream);
int gpp_plane_select_polled_workspace_bytes(int M, size_t* bytes);
int gpp_plane_select_polled(const uint16_t* keys, const uint16_t* errs, int O, int M, int64_t pitch, int K, int32_t* chosen,
                            uint64_t* trace, uint16_t* best, uint16_t* cur, int32_t* count, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-frame road-plane fit (csrc/road_fit.hip; DESIGN.md section 4.22 is the specification, utils/road_fit.py the host side and the NumPy
 * form): from a batch of LiDAR scans one plane per frame, in rectified camera coordinates -- the pool that gpp_poll_costs_u16 /
 * gpp_plane_select distil.  Exact integers: points are quantised once at GPP_ROAD_Q quanta per metre and every later quantity is an integer
 * below 2^53 or one rounded float64 operation of such integers, so every output equals the NumPy form and does not depend on the order of
 * lanes or atomics.  Four plain launches in stream order (points, score, winner, moments); no workspace; the 2 x 2 solve is the host's.
 * A second, third ... plane per frame: gpp_road_peel_i32 below takes the winner's inliers out and the three launches run again.
 *
 * The ragged batch: frame f owns the points [offsets[f], offsets[f + 1]) of `points` and the same rows of `q`.  offsets (F + 1) int32 is
 * DEVICE memory; the host passes what it knows of it, total = offsets[F] and max_points >= every frame's size.  A frame whose offsets
 * descend, leave [0, total] or span more than max_points is an empty frame to every kernel (kept 0, counts -1, winner -1, sums 0): nothing
 * is read or written outside [0, total).  F <= 65535 (chunk a dataset), max_points <= GPP_ROAD_MAX_POINTS = 2^20, max_points <= total
 * <= GPP_ROAD_MAX_TOTAL.
 *
 * gpp_road_points_i32: gate and quantise.  One workgroup per frame, chunks of 256 points, a stable compaction.
 *   points (total, 4) float32 x y z reflectance, 16-byte aligned; T (F, 12) float64: per frame R0_rect . Tr_velo_to_cam, rows of 4.
 *   per point and row r, in float64, every operation rounded:  v_r = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3],
 *   q_r = floor(v_r * 256.0 + 0.5);  kept iff |q_0| <= xq, |q_1| <= yq and 1 <= q_2 <= zq on the doubles (NaN and infinity fail).
 *   xq, yq, zq: the region in quanta, 0 <= xq <= 10240, 0 <= yq <= 2048, 1 <= zq <= 20480 (40 m, 8 m, 80 m).  These caps are what bound
 *   everything below: a difference of two points < 2^15.4 per axis, a cross-product component < 2^33, n . (p - p0) < 2^51.
 *   q (total, 3) int32: the kept points of frame f, IN THE SCAN'S ORDER, at rows offsets[f] ... offsets[f] + kept[f]; the rest of the
 *   frame's rows are left untouched.  kept (F) int32.
 *
 * gpp_road_score: count (F, H) int32.  mix(u): u ^= u >> 16, u *= 0x7feb352d, u ^= u >> 15, u *= 0x846ca68b, u ^= u >> 16 (uint32).
 *   hypothesis h of frame f with m = kept[f]:  r_k = mix(mix(mix(seed + frame_id[f]) + h) + k), i_k = (uint64(r_k) * m) >> 32, k = 0 1 2;
 *   n = (p_i1 - p_i0) x (p_i2 - p_i0), d0 = n . p_i0 (integers); nn = (nx nx + ny ny) + nz nz in float64, every operation rounded;
 *   valid iff m >= 3, nn > 0, ny ny >= c2 nn and hlo2 nn <= d0 d0 <= hhi2 nn (float64 products of the integers' exact conversions).
 *   count = the number of kept points p of the frame with dot dot <= tq2 nn, dot = n . p - d0 (an integer, converted exactly);
 *   an invalid hypothesis: count = -1.  frame_id (F) uint32 and seed make the draws: chunking a dataset never changes a frame's draws.
 *   c2 in [0, 1], 0 <= hlo2 <= hhi2, tq2 >= 0 (cos^2 of the largest tilt, the height band and the threshold in quanta, squared).
 *   Grid: ceil(H / 256) x min(ceil(max_points / GPP_ROAD_SLAB), 64) x F workgroups, one lane per hypothesis; a workgroup walks every
 *   64th slab of GPP_ROAD_SLAB points, staged in LDS as float64 and read as a broadcast, and adds the lane's count with one atomicAdd.
 *   `count` is cleared first.
 *   H <= GPP_ROAD_MAX_HYPOTHESES.  F == 0 or H == 0: GPP_OK, nothing launched.
 *
 * gpp_road_winner: per frame the largest count and the FIRST h among equals.  winner (F) int32: that h, or -1 when the count is below
 *   min_inliers (>= 1) or no hypothesis is valid; inliers (F) int32: the largest count, 0 when no hypothesis is valid.
 *
 * gpp_road_moments: sums (F, 10) int64, 8-byte aligned: N, Sx, Sy, Sz, Sxx, Sxz, Szz, Sxy, Szy, Syy over the inliers (the rule of
 *   gpp_road_score) of the winner's plane, recomputed from its three draws; zero for a frame without a winner.  ceil(max_points / 2048) x F
 *   workgroups, 64-bit integer atomics.  A frame has at most 2^20 points: every sum < 2^50.
 *
 * gpp_road_peel_i32 (several planes per frame): q_out (total, 3) int32, the layout of q_in: the kept points of
 *   frame f that are NOT inliers of `winner[f]`'s plane, IN THEIR ORDER (a stable compaction), at rows offsets[f] ... offsets[f] +
 *   kept_out[f]; the rest of the frame's rows are left untouched.  kept_out (F) int32.  The inlier test is gpp_road_moments', operation for
 *   operation, on the plane recomputed from the winner's three draws under `seed`: kept_in[f] - kept_out[f] equals that launch's N for
 *   every frame with a winner.  A frame without a winner (winner < 0 or >= H) is finished: kept_out = 0, nothing written.  A winner whose
 *   plane has nn = 0 or whose frame has fewer than three points (hand-set only: the winner launch never names one) has no inliers, here
 *   as in gpp_road_moments: every kept point survives.  The next round's score / winner / moments run unchanged on (q_out, kept_out) with
 *   the round's seed, seed_r = seed + r * 0x9e3779b9 (mod 2^32), made by the host.
 *   q_out and q_in are distinct buffers whose (total, 3) ranges do not overlap (GPP_ERR_BAD_ARG otherwise): the host ping-pongs two.
 *   Three plain launches, no atomics: (a) ceil(max_points / GPP_ROAD_PEEL_BLOCK) x F workgroups count their block's survivors into the
 *   workspace; (b) one workgroup per frame scans its block counts in place (up to 512 of them, in chunks of 256 with a carry) and writes
 *   kept_out; (c) the grid of (a) recomputes the mask and places every survivor: a ballot per wavefront and an LDS prefix across the four.
 *   workspace: gpp_road_peel_workspace_bytes(F, max_points) bytes, 4-byte aligned like q_in, q_out and kept_out; too small:
 *   GPP_ERR_WORKSPACE.  F == 0: GPP_OK, nothing launched.
 *
 * Null pointer, a size or bound outside the ranges above: GPP_ERR_BAD_ARG; alignment: GPP_ERR_ALIGN; nothing is launched in these cases.
 * ---------------------------------------------------------------------------------------- */
#define GPP_ROAD_Q 256
#define GPP_ROAD_MAX_XQ 10240
#define GPP_ROAD_MAX_YQ 2048
#define GPP_ROAD_MAX_ZQ 20480
#define GPP_ROAD_SLAB 512
#define GPP_ROAD_MAX_POINTS (1 << 20)
#define GPP_ROAD_MAX_TOTAL (1 << 30)
#define GPP_ROAD_MAX_HYPOTHESES (1 << 20)
int gpp_road_points_i32(const float* points, const int32_t* offsets, const double* T, int F, int total, int max_points,
                        int xq, int yq, int zq, int32_t* q, int32_t* kept, void* stream);
int gpp_road_score(const int32_t* q, const int32_t* offsets, const int32_t* kept, const uint32_t* frame_id, uint32_t seed,
                   int F, int total, int max_points, int H, double c2, double hlo2, double hhi2, double tq2, int32_t* count, void* stream);
int gpp_road_winner(const int32_t* count, int F, int H, int min_inliers, int32_t* winner, int32_t* inliers, void* stream);
int gpp_road_moments(const int32_t* q, const int32_t* offsets, const int32_t* kept, const uint32_t* frame_id, uint32_t seed,
                     const int32_t* winner, int F, int total, int max_points, int H, double tq2, int64_t* sums, void* stream);
#define GPP_ROAD_PEEL_BLOCK 2048
int gpp_road_peel_workspace_bytes(int F, int max_points, size_t* bytes);
int gpp_road_peel_i32(const int32_t* q_in, const int32_t* offsets, const int32_t* kept_in, const uint32_t* frame_id, uint32_t seed,
                      const int32_t* winner, int F, int total, int max_points, int H, double tq2,
                      int32_t* q_out, int32_t* kept_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The --save-images composite on the device (csrc/draw.hip; DESIGN.md section 4.14 is the specification, utils/visualization.py its host
 * form): per image the 2-D picture (boxes, keypoint markers, score captions) over the 3-D picture (projected cuboids, residual captions),
 * from the rows of gpp_pose_f32 and the raw uint8 BGR frames.  Two launches on one stream: gpp_draw_build, then gpp_draw_raster.
 *
 * gpp_draw_build: one thread per detection, one workgroup per image, float64.
 *   rows (B, D, GPP_POSE_COLS) float32: the rows of gpp_pose_f32 (columns 0-24 are read).
 *   P (B, 3, 4) float64, device: per image the calibration in raw-image pixels.
 *   score_thr: the rows with score > score_thr are drawn (a NaN score is not), in row order, numbered k = 0 .. n-1.
 *   prims: gpp_draw_workspace_bytes' prims_bytes, 16-byte aligned.  Image b owns the records [b D 26, (b + 1) D 26) and fills the first
 *   26 n of them, in painter's order: top picture [0, 3n) = box, circle, caption of every detection, [3n, 13n) = the ten marker lines of
 *   every detection (3 up-triangle at m, 4 square at r, 3 down-triangle at t); bottom picture [13n, 26n) = caption and twelve edges of
 *   every detection.  A primitive that is not drawn (a coordinate not finite or |c| >= 2^20, an orientation class outside 0..3, a
 *   cuboid behind the camera ...) keeps its slot as GPP_DRAW_NONE.
 *   counts (B, GPP_DRAW_COUNT_WORDS) int32: n, the number of records (26 n), the index of the image's first record, 0.
 *
 *   a record = GPP_DRAW_PRIM_WORDS int32 words
 *    0        kind: GPP_DRAW_NONE / LINE / DASHED / RECT / CIRCLE / CAPTION
 *    1        picture: 0 = top (output rows [0, h)), 1 = bottom (rows [h, 2h)); coordinates are the picture's own
 *    2 -  5   x0 y0 x1 y1: the endpoints (LINE, DASHED); the sorted corners x0 <= x1, y0 <= y1 (RECT); the centre and 0 0 (CIRCLE);
 *             the bottom-left corner of the first glyph, the number of characters and 0 (CAPTION).  |coordinate| < 2^20
 *    6        colour: channel 0 | channel 1 << 8 | channel 2 << 16 (unused by a CAPTION: black under white)
 *    7 - 10   bounding box xmin ymin xmax ymax (inclusive) of every pixel the record can paint
 *   11 - 15   CAPTION: up to GPP_DRAW_CAPTION_MAX characters, one byte each, as indices into "0123456789.:- "
 *
 * gpp_draw_raster: one workgroup per 64 x 4 tile of output pixels, one pixel per thread; a later record overwrites an earlier one.
 *   frames_u8 (B slots of Hr Wr 3 bytes), out_u8 (B slots of 2 Hr Wr 3 bytes): the slot convention of the ragged uint8 canvas -- image b
 *   sits densely (row pitch 3 w_b) at the start of slot b; raw_hw (B, 2) int32, device: its height and width (clamped to Hr, Wr).  A
 *   uniform batch (B, Hr, Wr, 3) is the same call.  Bytes of a slot beyond the image's own 2 h_b x w_b x 3 are not written.
 *   prims, counts: as gpp_draw_build leaves them (or any table of valid records with bounding boxes that hold what they paint).
 *   workspace: gpp_draw_workspace_bytes' workspace_bytes, 4-byte aligned; afterwards (B, 4) int32: the records examined, the records
 *   of an unknown kind or picture (ignored; 0 for a table of gpp_draw_build), 2 h_b, w_b.
 *
 *   Null pointer, negative size, misaligned pointer: GPP_ERR_BAD_ARG, nothing launched.  B == 0 (or, for the raster, an empty frame):
 *   GPP_OK, nothing launched.  D == 0: gpp_draw_build writes counts of 0 (rows and prims may be null) and the raster copies the frames.
 * ---------------------------------------------------------------------------------------- */
#define GPP_DRAW_PRIM_WORDS 16
#define GPP_DRAW_PRIMS_PER_DET 26
#define GPP_DRAW_COUNT_WORDS 4
#define GPP_DRAW_CAPTION_MAX 20
#define GPP_DRAW_NONE 0
#define GPP_DRAW_LINE 1
#define GPP_DRAW_DASHED 2
#define GPP_DRAW_RECT 3
#define GPP_DRAW_CIRCLE 4
#define GPP_DRAW_CAPTION 5
int gpp_draw_workspace_bytes(int B, int D, size_t* prims_bytes, size_t* workspace_bytes);
int gpp_draw_build(const float* rows, const double* P, int B, int D, float score_thr, void* prims, int32_t* counts, void* stream);
int gpp_draw_raster(const uint8_t* frames_u8, const int32_t* raw_hw, int Hr, int Wr, const void* prims, const int32_t* counts,
                    int B, uint8_t* out_u8, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Range audit of dtype='f16x3' (csrc/audit.hip; opt-in: RetinaNet3D(range_audit=True)): the largest |x| of
 * every channel of one NHWC map, read in one of the three forms an x3 convolution reads its activation operand in.
 *
 *   in      the map's buffer; pixel m starts at element m * pitch of it, the audited channels are [c_off, c_off + C) of every pixel
 *           (pitch >= c_off + C: a channel prefix or slice of a wider buffer).  Elements are float32-sized in every layout.
 *   layout  GPP_ABSMAX_F32         plain float32 rows; any C >= 1 (16-byte loads when C, pitch and the first channel allow them)
 *           GPP_ABSMAX_SPLIT_F16   pre-split rows (gpp_conv_desc.x3_split): every 32 channels are 128 bytes [32 IEEE halves hi | 32 lo],
 *           GPP_ABSMAX_SPLIT_BF16  or bf16 halves; the value of a channel is float(hi) + float(lo).  C, pitch and c_off multiples of 32
 *                                  and `in` 128-byte aligned, else GPP_ERR_BAD_ARG / GPP_ERR_ALIGN.
 *   out     uint32 [C], device: out[c] = max(out[c], bits(|x[m, c_off + c]|)) over the M pixels.  Non-negative floats order like their
 *           bit patterns, so this is an integer maximum (one relaxed atomic per channel per workgroup): independent of the order of
 *           arrival, a NaN wins over every number and stays visible, and a launch ADDS to what earlier launches left (two half batches,
 *           five pyramid levels).  The caller clears the table: gpp_absmax_clear (a memset on the stream).
 *   Null pointer, C <= 0, M < 0, pitch < c_off + C, unknown layout, reserved != 0: GPP_ERR_BAD_ARG, nothing launched (checked on the
 *   host, no device needed).  M == 0: GPP_OK, nothing launched.
 * ---------------------------------------------------------------------------------------- */
#define GPP_ABSMAX_F32 1
#define GPP_ABSMAX_SPLIT_F16 2
#define GPP_ABSMAX_SPLIT_BF16 3
typedef struct gpp_absmax_desc {
    const void* in; uint32_t* out;
    int64_t M, pitch;
    int32_t C, c_off, layout, reserved;
} gpp_absmax_desc;
typedef struct gpp_absmax_clear_desc { uint32_t* table; int64_t n; } gpp_absmax_clear_desc;
int gpp_channel_absmax(const gpp_absmax_desc* desc, void* stream);
int gpp_absmax_clear(uint32_t* table, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Plan execution: one call enqueues a whole predict_on_batch (every kernel of the graph that
 * models/retinanet.py:359-422 `retinanet_bbox` builds) from a host array of descriptors.
 * The runner holds no state: the caller (Python) keeps the descriptors and buffers alive.
 * Ops whose `tag` is non-zero are bracketed by HIP events when `events` is given: the k-th
 * tagged op records events[2k] before and events[2k+1] after its launch, on `stream`
 * (this is how bench.py measures the dominant kernel live inside the timed region).
 * ---------------------------------------------------------------------------------------- */
#define GPP_OP_STEM 1
#define GPP_OP_MAXPOOL 2
#define GPP_OP_CONV 3
#define GPP_OP_RELU 4
#define GPP_OP_DETECT 5
#define GPP_OP_POLL 6
#define GPP_OP_BOTTLENECK_TAIL 7
#define GPP_OP_DETECT_CANDIDATES 8   /* gpp_detect_desc; stages of GPP_OP_DETECT, see gpp_detect_stages_f32 */
#define GPP_OP_DETECT_SELECT 9
#define GPP_OP_DETECT_EMIT 10
/* (11: the three-layer tail of round 2, removed in round 3 -- measured slower than its separate launches) */
#define GPP_OP_DETECT_OSF 12             /* gpp_detect_desc -> gpp_detect_osf_f32 */
#define GPP_OP_STEM_POOL 13              /* gpp_stem_desc with out = the pooled map -> gpp_stem_pool_fused_mfma (GPP_BF16 / GPP_F16) / gpp_stem_pool_fused_x3 (GPP_F16X3 / GPP_BF16X3) */
#define GPP_OP_BOTTLENECK_BLOCK 16       /* gpp_block_desc -> gpp_bottleneck_block; with form = 1 a gpp_block_proj_desc -> gpp_bottleneck_block_proj */
#define GPP_OP_MAXPOOL_PAD 17            /* gpp_dense_pool_desc -> gpp_maxpool3x3s2_pad_f32 (DenseNet pool1) */
#define GPP_OP_AVGPOOL 18                /* gpp_dense_pool_desc -> gpp_avgpool2x2_f32 (DenseNet transitions) */
#define GPP_OP_POSE 19                   /* gpp_pose_desc -> gpp_pose_f32 (opt-in: RetinaNet3D(pose=True)) */
#define GPP_OP_CUBOID_NMS 20             /* gpp_cuboid_nms_desc -> gpp_cuboid_nms_f64 behind GPP_OP_POSE (opt-in: RetinaNet3D(pose=True, cuboid_nms=(metric, threshold))) */
#define GPP_OP_CONV_PREACT 32            /* gpp_preact_desc -> gpp_conv2d_preact (DenseNet); kinds 0..255 exist */
#define GPP_OP_MOBILENET_STEM 33         /* gpp_mobilenet_stem_desc -> gpp_mobilenet_stem */
#define GPP_OP_MOBILENET_BLOCK 34        /* gpp_mobilenet_block_desc -> gpp_mobilenet_block */
#define GPP_OP_ABSMAX 35                 /* gpp_absmax_desc -> gpp_channel_absmax (opt-in: RetinaNet3D(range_audit=True)) */
#define GPP_OP_ABSMAX_CLEAR 36           /* gpp_absmax_clear_desc -> gpp_absmax_clear: the first op of an audit plan */
#define GPP_OP_STEM_RAGGED 37             /* gpp_ragged_stem_desc -> gpp_stem_conv7x7_bn_relu_ragged / _mfma_ragged / _x3_rc_ragged (by dtype, as GPP_OP_STEM) */
#define GPP_OP_STEM_POOL_RAGGED 38        /* gpp_ragged_stem_desc with out = the pooled map -> gpp_stem_pool_fused_mfma_ragged / gpp_stem_pool_fused_x3_ragged */
#define GPP_OP_MAXPOOL_RAGGED 39          /* gpp_ragged_pool_desc -> gpp_maxpool3x3s2_same_ragged */
#define GPP_OP_DETECT_CANDIDATE_PIXELS 40  /* gpp_candidate_pixels_desc: GPP_OP_DETECT_CANDIDATES, then gpp_detect_pixel_lists on the same stream */
/* (14, 15: the Winograd F(2, 3) form of the tower layers of round 5 -- built, measured at -2 % of the step, shelved in round 6:
   tools/experiments/winograd/) */
/* Optional concurrency inside a plan: `kind | GPP_OP_LANE(l)` (l = 1, 2) enqueues the op on a library-owned side stream
   that forks from the caller's stream at the first op of that lane; `kind | GPP_OP_JOIN` on a lane-0 op makes it wait
   for every open lane (the end of the plan joins too, and so does every error return: a failed gpp_plan_run leaves no forked work
   un-joined).  GPP_OP_JOIN on a side-lane op is GPP_ERR_BAD_ARG.  The caller orders the ops so that each lane only depends on
   what was enqueued before its fork.  The side streams belong to the DEVICE (one pair per device ordinal, made on first use): plans
   enqueued on different caller streams of one device share them, so their side-lane work is ordered plan after plan.
   Used for the projection shortcuts, the half-batch chains of res3-res5, the small FPN launches and the detection selection. */
#define GPP_OP_LANE(l) ((l) << 8)
#define GPP_OP_JOIN 0x10000
/* on a side-lane op: the lane first waits for everything enqueued on the caller's stream so far (a second fork point) */
#define GPP_OP_SYNC 0x20000

/* Optional stage label of an op, bits 20-23 of `kind`: with GPP_ROCTX=1 in the environment gpp_plan_run opens a roctx range ("gpp:stem", "gpp:backbone",
   "gpp:fpn", "gpp:heads", "gpp:decode", "gpp:polling", "gpp:pose", "gpp:cuboid_nms") around each run of consecutive ops with the same label (rocprofv3 --marker-trace); 0 = none.
   The marker library is looked up at run time; without the variable nothing is loaded.  GPP_ROCTX=2 additionally synchronises the device where a range opens and
   closes: a range's duration in the marker trace is then its stage's time on the device (tools/roctx_stages.sh); a measuring mode, not a production one. */
#define GPP_OP_STAGE(s) (((s) & 15) << 20)
#define GPP_STAGE_STEM 1
#define GPP_STAGE_BACKBONE 2
#define GPP_STAGE_FPN 3
#define GPP_STAGE_HEADS 4
#define GPP_STAGE_DECODE 5
#define GPP_STAGE_POLLING 6
#define GPP_STAGE_POSE 8
#define GPP_STAGE_AUDIT 9                /* "gpp:audit": the GPP_OP_ABSMAX launches of an audit plan */
#define GPP_STAGE_CUBOID_NMS 10          /* "gpp:cuboid_nms": the GPP_OP_CUBOID_NMS launch behind the pose stage */

typedef struct gpp_stem_desc { const float* in; const void* weight; const float* bias; void* out;
                               int32_t dtype, B, H, W; uint64_t* range_counter; /* GPP_F16X3: see gpp_stem_conv7x7_bn_relu_x3_rc; NULL otherwise */
                             } gpp_stem_desc;   /* weight: packed f16 image (MFMA stem); GPP_F32: float32 [147][64]; GPP_F16X3: gpp_stem_pack_weights_f16x3 */
typedef struct gpp_pool_desc { const void* in; void* out; int32_t dtype, B, H, W, C, reserved; } gpp_pool_desc;
/* a batch of one height class: stem.H = 4 Hp canvas rows (pool.H = 2 Hp map rows); heights = int32 [B] in device memory, the IMAGE heights */
typedef struct gpp_ragged_stem_desc { gpp_stem_desc stem; const int32_t* heights; int32_t Hp, reserved; } gpp_ragged_stem_desc;
typedef struct gpp_ragged_pool_desc { gpp_pool_desc pool; const int32_t* heights; int32_t Hp, reserved; } gpp_ragged_pool_desc;
typedef struct gpp_relu_desc { const void* in; void* out; int64_t in_bstride, out_bstride, count;
                               int32_t dtype, B; } gpp_relu_desc;
typedef struct gpp_detect_desc {
    const float* cls_logits; const float* regression; const float* regression_dim; const float* anchors;
    float* boxes; float* dims; float* scores; int32_t* labels; int32_t* orientations;
    int32_t* anchor_index; int32_t* counts; void* workspace;
    size_t workspace_bytes; int64_t n_anchors;
    int32_t B, num_base_anchors, fused_layout, max_det;
    float score_thr, iou_thr;
} gpp_detect_desc;
typedef struct gpp_candidate_pixels_desc { const gpp_detect_desc* detect; gpp_pixel_list_desc lists; } gpp_candidate_pixels_desc;
typedef struct gpp_poll_desc {
    const float* boxes; const float* dims; const int32_t* orient; const float* P_inv; const float* planes;
    float* keypoints; float* keyplanes; float* residuals; int32_t* best_idx; void* workspace;
    size_t workspace_bytes;
    int32_t B, D, N, planes_batched;
    float thr; int32_t reserved;
} gpp_poll_desc;

typedef struct gpp_pose_desc {
    const float* boxes; const float* dims; const float* scores; const int32_t* labels; const int32_t* orientations;
    const float* keypoints; const float* residuals; const float* frame_info; float* rows; int32_t* counts;
    int32_t B, D;
    float score_thr; int32_t reserved;
} gpp_pose_desc;

/* in place on the pose op's rows and counts: rows = gpp_pose_desc.rows, counts = gpp_pose_desc.counts */
typedef struct gpp_cuboid_nms_desc {
    float* rows; int32_t* counts; int32_t* suppressor;
    double iou_thr;
    int32_t B, D, metric, reserved;
} gpp_cuboid_nms_desc;

typedef struct gpp_tail_desc { const gpp_conv_desc* conv3x3; const gpp_conv_desc* conv1x1; int32_t tile_rows, reserved; } gpp_tail_desc;
/* form: 0 = the three layers (the shortcut is conv1x1_c->residual); 1 = the record is a gpp_block_proj_desc (the same fields, then the fourth layer) */
typedef struct gpp_block_desc { const gpp_conv_desc* conv1x1_a; const gpp_conv_desc* conv3x3_b; const gpp_conv_desc* conv1x1_c; int32_t tile, form; } gpp_block_desc;
typedef struct gpp_block_proj_desc { gpp_block_desc block; const gpp_conv_desc* conv1x1_proj; } gpp_block_proj_desc;

typedef struct gpp_preact_desc { const gpp_conv_desc* conv; const float* in_scale; const float* in_shift; } gpp_preact_desc;
typedef struct gpp_dense_pool_desc { const float* in; float* out; int32_t B, H, W, C, pad, out_pitch; } gpp_dense_pool_desc;   /* pad: max-pool only */

typedef struct gpp_plan_op { int32_t kind; int32_t tag; const void* desc; } gpp_plan_op;

int gpp_plan_run(const gpp_plan_op* host_ops, int n_ops, void* stream, void* const* events, int n_events);

/* HIP events for callers without HIP headers (bench.py): timing enabled, host handles. */
int gpp_event_create(void** event);
int gpp_event_destroy(void* event);
int gpp_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */

#ifdef __cplusplus
}
#endif

#endif /* GPP_H_ */
