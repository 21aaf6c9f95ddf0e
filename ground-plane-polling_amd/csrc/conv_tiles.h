// The block-tile catalogue of the implicit-GEMM convolution: every value of gpp_conv_desc.tile_hint, stated ONCE.  Host code only.
//
// Derived from it: the switches of dispatch<DT> / dispatch_gather<DT> / dispatch_preact<DT> (conv_igemm_impl.h), the candidate lists of
// gpp_conv2d_tile_candidates / gpp_conv2d_preact_tile_candidates and the autotuners (conv_igemm.hip).  A code in the table that this
// element type or input form does not own answers GPP_ERR_UNSUPPORTED (the 16-bit types answer GPP_ERR_BAD_ARG to the x3 types' codes, as
// they always have); a code that is not in the table answers GPP_ERR_BAD_ARG.  tests/test_tile_table_cpu.py pins all of it, without a device.
#ifndef GPP_CONV_TILES_H_
#define GPP_CONV_TILES_H_

#include <stdint.h>

#include "gpp.h"

namespace gpp_tiles {

// the loop / grid an entry runs with
enum Form {
    PLAIN,       // the two-buffer ring, loads and MFMAs of one K-step back to back
    PIPE,        // 1000000 + ...: the software-pipelined main loop (x3 types: the three-phase loop, pre-split input maps only)
    DUAL,        // 2256256: 256 x 256 tiles + 512 x 128 tiles for the last 128 columns in one grid (C_out = 256 k + 128)
    MIX,         // 3000000 + BMA * 1000 + BMB: 256-column tiles of two heights in one grid
    WS,          // 4000000 + ...: the weight-stationary persistent 1 x 1
    DEEP,        // 5000000 + ...: the plain loop on a four-deep ring
    GATHER,      // 6000000 / 7000000 + ...: the gathered-row form (gpp_conv_desc.gather_rows), two- / four-deep ring
    PREACT,      // gpp_conv2d_preact
    GATHER_PIPE, // 8000000 + ...: the gathered-row form into a pre-split map (a layer between two convolutions): the three-phase pipelined loop
};

// who has an instantiation of it
enum Owner {
    ALL,         // every element type
    ALL_X3IN,    // every element type; the x3 types on a pre-split input map only
    B16,         // GPP_BF16 / GPP_F16
    NOT_F32,     // the 16-bit types and the x3 types
    X3,          // the x3 types
    X3IN,        // the x3 types on a pre-split input map (x3_split & GPP_X3_IN)
};

struct Entry {
    int code, form, owner;
    int bm, bn;             // block tile (MIX: bm = BMA, bn = BMB; its tiles are 256 columns wide)
    int wm, wn, stages;     // wavefront layout, depth of the LDS ring
};

// T(code, form, owner, BM, BN, WM, WN, STAGES): a candidate of the dense / gathered form, in the order the autotuner times them (its strict
// `<` lets the order decide ties, and tests read the order); X(...): reachable, never a candidate -- the legacy aliases and the three-deep
// experiment; P(...): the tiles of gpp_conv2d_preact, in its tuner's order.  (Round 2's loader-wavefront form, 3064128 ..., 1.5 - 2x slower
// on every layer it was built for (profiles/r2/ring_kernel.txt), is no longer part of the library.)
#define GPP_CONV_TILES(T, X, P)                                                                                                          \
    T(64064, PLAIN, ALL, 64, 64, 2, 2, 2)                                                                                                \
    T(96064, PLAIN, ALL, 96, 64, 2, 2, 2)                                                                                                \
    T(128064, PLAIN, ALL, 128, 64, 2, 2, 2)                                                                                              \
    T(160064, PLAIN, ALL, 160, 64, 2, 2, 2)                                                                                              \
    T(192064, PLAIN, ALL, 192, 64, 2, 2, 2)                                                                                              \
    T(64128, PLAIN, ALL, 64, 128, 2, 2, 2)                                                                                               \
    T(96128, PLAIN, ALL, 96, 128, 2, 2, 2)                                                                                               \
    T(128128, PLAIN, ALL, 128, 128, 2, 2, 2)                                                                                             \
    T(160128, PLAIN, ALL, 160, 128, 2, 2, 2)                                                                                             \
    T(192128, PLAIN, ALL, 192, 128, 2, 2, 2)                                                                                             \
    T(224128, PLAIN, ALL, 224, 128, 2, 2, 2)                                                                                             \
    T(1128128, PIPE, NOT_F32, 128, 128, 2, 2, 2)                                                                                         \
    T(1192128, PIPE, NOT_F32, 192, 128, 2, 2, 2)                                                                                         \
    T(1128256, PIPE, NOT_F32, 128, 256, 2, 4, 2)                                                                                         \
    T(1160256, PIPE, X3IN, 160, 256, 2, 4, 2)            /* (224 / 160 rows: staged as 256 / 192, see stage_rows) */                     \
    T(1192256, PIPE, NOT_F32, 192, 256, 2, 4, 2)                                                                                         \
    T(1224256, PIPE, X3IN, 224, 256, 2, 4, 2)                                                                                            \
    /* 8 wavefronts, one workgroup per CU: half the L2 -> LDS traffic per FLOP.  The 16-bit types run it with the pipelined loop under  \
       this plain code too (tile_pipelined below); the x3 types with the plain loop, on either input form */                            \
    T(256256, PLAIN, NOT_F32, 256, 256, 2, 4, 2)                                                                                         \
    T(1256256, PIPE, X3IN, 256, 256, 2, 4, 2)                                                                                            \
    /* N-remainder tiles (4 x 1 wavefronts, wave tile BM/4 x 160): layers whose C_out is far from a multiple of 128 (regression         \
       outputs: 144 -> 160 instead of 256 columns; measured 200 -> 162 us); 96 columns for the classification logits */                 \
    T(128160, PLAIN, ALL, 128, 160, 4, 1, 2)                                                                                             \
    T(192160, PLAIN, ALL_X3IN, 192, 160, 4, 1, 2)        /* (x3, float32 input: 3 registers over the budget -- no such form) */          \
    T(1192160, PIPE, B16, 192, 160, 4, 1, 2)                                                                                             \
    T(1128160, PIPE, NOT_F32, 128, 160, 4, 1, 2)                                                                                         \
    T(2256256, DUAL, NOT_F32, 256, 256, 2, 4, 2)                                                                                         \
    T(1192096, PIPE, NOT_F32, 192, 96, 4, 1, 2)                                                                                          \
    T(3256224, MIX, X3IN, 256, 224, 2, 4, 2)                                                                                             \
    T(3192160, MIX, X3IN, 192, 160, 2, 4, 2)                                                                                             \
    T(4128064, WS, X3IN, 128, 64, 2, 4, 4)                                                                                               \
    T(4064064, WS, X3IN, 64, 64, 2, 4, 4)                                                                                                \
    T(4128128, WS, X3IN, 128, 128, 2, 4, 4)                                                                                              \
    T(4064128, WS, X3IN, 64, 128, 2, 4, 4)                                                                                               \
    /* for launches of at most one workgroup per CU (deep K and small M, batch 1), bound by the latency of their own tile loads: three   \
       K-steps of LDS-DMA in flight; where workgroups would share a CU the footprint loses (round 2: 1.6 x slower at B = 8) */          \
    T(5064064, DEEP, X3IN, 64, 64, 2, 2, 4)                                                                                              \
    T(5096064, DEEP, X3IN, 96, 64, 2, 2, 4)                                                                                              \
    T(5064128, DEEP, X3IN, 64, 128, 2, 2, 4)                                                                                             \
    T(5096128, DEEP, X3IN, 96, 128, 2, 2, 4)                                                                                             \
    T(5128128, DEEP, X3IN, 128, 128, 2, 2, 4)                                                                                            \
    /* the x3 types spend 3 MFMAs per fragment pair: with 4-wavefront tiles their LDS traffic equals their matrix time; the             \
       8-wavefront 256-column tiles (plain two-buffer loop) halve the LDS bytes per MFMA */                                             \
    T(128256, PLAIN, X3, 128, 256, 2, 4, 2)                                                                                              \
    T(192256, PLAIN, X3, 192, 256, 2, 4, 2)                                                                                              \
    /* gathered rows: short and narrow, so that a few thousand rows still field a few hundred workgroups (64 x 160, 4 x 1 layout: the   \
       144 regression channels); at most about one workgroup per CU, bound by its own loads' latency: hence the four-deep ring */       \
    T(6064064, GATHER, ALL, 64, 64, 2, 2, 2)                                                                                             \
    T(6032064, GATHER, ALL, 32, 64, 2, 2, 2)                                                                                             \
    T(6064160, GATHER, ALL, 64, 160, 4, 1, 2)                                                                                            \
    T(7064064, GATHER, ALL, 64, 64, 2, 2, 4)                                                                                             \
    T(7032064, GATHER, ALL, 32, 64, 2, 2, 4)                                                                                             \
    T(7064160, GATHER, ALL, 64, 160, 4, 1, 4)                                                                                            \
    /* gathered rows of a 256 k-column tower layer (pre-split maps, the three-phase loop; a persistent grid of one workgroup per CU that    \
       takes the listed rows' tiles in order).  The host cannot know the count, and a fixed height pays up to a whole round for a few rows  \
       past a multiple of the chip: 8000256 takes the height on the device (gather_pipe_rows below), and is the one the tuner and the      \
       plans use; the fixed heights are reachable (tests, tools/bench_sparse_tower.py) */                                                   \
    T(8000256, GATHER_PIPE, X3IN, 0, 256, 2, 4, 2)                                                                                       \
    X(8128256, GATHER_PIPE, X3IN, 128, 256, 2, 4, 2)                                                                                     \
    X(8160256, GATHER_PIPE, X3IN, 160, 256, 2, 4, 2)                                                                                     \
    X(8192256, GATHER_PIPE, X3IN, 192, 256, 2, 4, 2)                                                                                     \
    X(8224256, GATHER_PIPE, X3IN, 224, 256, 2, 4, 2)                                                                                     \
    X(8256256, GATHER_PIPE, X3IN, 256, 256, 2, 4, 2)                                                                                     \
    X(64, PLAIN, ALL, 128, 64, 2, 2, 2)                                                                                                  \
    X(128, PLAIN, ALL, 128, 128, 2, 2, 2)                                                                                                \
    X(256, PLAIN, B16, 256, 128, 4, 2, 3)                /* 3-deep ring, experiments only */                                             \
    X(512, PLAIN, B16, 256, 256, 2, 4, 2)                                                                                                \
    P(64064, PREACT, ALL, 64, 64, 2, 2, 2)                                                                                               \
    P(128064, PREACT, ALL, 128, 64, 2, 2, 2)                                                                                             \
    P(64128, PREACT, ALL, 64, 128, 2, 2, 2)                                                                                              \
    P(128128, PREACT, ALL, 128, 128, 2, 2, 2)                                                                                            \
    P(192128, PREACT, ALL, 192, 128, 2, 2, 2)

#define GPP_TILE_ENTRY(code, form, owner, bm, bn, wm, wn, stages) {code, gpp_tiles::form, gpp_tiles::owner, bm, bn, wm, wn, stages},
#define GPP_TILE_NONE(...)

constexpr bool owner_has(int owner, bool f32_storage, bool x3)
{
    return owner == ALL || owner == ALL_X3IN || (owner == B16 && !f32_storage) || (owner == NOT_F32 && (!f32_storage || x3)) ||
           ((owner == X3 || owner == X3IN) && x3);
}

// x3 types: only the plain loops read a float32 input map (and split it on the way into LDS); every other form wants it pre-split
constexpr bool x3_wants_split_input(int form, int owner)
{
    return owner == X3IN || owner == ALL_X3IN || (form != PLAIN && form != GATHER && form != PREACT);
}

// the gathered-row form into a pre-split map: x3 types, pre-split input and output, stride 1, no shortcut, never split, whole 256-column tiles
inline bool gather_pipe_can_run(const gpp_conv_desc& d)
{
    return (d.dtype == GPP_BF16X3 || d.dtype == GPP_F16X3) && (d.x3_split & (GPP_X3_IN | GPP_X3_OUT)) == (GPP_X3_IN | GPP_X3_OUT) && !d.out_f32 &&
           d.stride == 1 && !d.residual && d.split_k <= 1 && d.C_out > 0 && d.C_out % 256 == 0;
}

// ... and the height its 8000256 code runs with, from the listed rows of every group (host and device: the kernel evaluates it on the counts it
// finds).  One workgroup of any of these heights fills a compute unit, so a grid costs rounds x rows x (time per row of a tile of that
// height): measured on the 512 -> 512 tower layer, a round takes 1.25 us per row with 128-row tiles and 0.98 with 256-row ones (the weight
// tile's traffic is shared by more rows; profiles/sparse_tower/crossover.txt) -- a straight line between the two, in 1/128ths.  Ties go to
// the SHORTER tile.  Heights: 128 .. 256 in steps of 32.  gather_pipe_tiles: the row tiles x column tiles the listed rows take at a height.
constexpr int kGatherPipeMinRows = 128, kGatherPipeMaxRows = 256, kGatherPipeCus = 256;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline long long gather_pipe_tiles(const int (&counts)[GPP_MAX_GROUPS], int n_groups, int n_tiles, int bm)
{
    long long tiles = 0;
    for (int g = 0; g < GPP_MAX_GROUPS; ++g) tiles += g < n_groups ? (counts[g] + bm - 1) / bm : 0;
    return tiles * n_tiles;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int gather_pipe_rows(const int (&counts)[GPP_MAX_GROUPS], int n_groups, int n_tiles)
{
    int best = 0;
    long long best_cost = 0;
    for (int bm = kGatherPipeMinRows; bm <= kGatherPipeMaxRows; bm += 32) {
        const long long rounds = (gather_pipe_tiles(counts, n_groups, n_tiles, bm) + kGatherPipeCus - 1) / kGatherPipeCus;
        const long long cost = rounds * bm * (12416 - 17 * bm);          // (128 rows: 80 / 64 us per row, 256 rows: 63 / 64)
        if (best == 0 || cost < best_cost) { best = bm; best_cost = cost; }
    }
    return best;
}

constexpr bool tile_pipelined(int form, int bm, int bn, bool f32_storage) { return form == PIPE || (!f32_storage && form == PLAIN && bm == 256 && bn == 256); }

// ---- hard eligibility: what a form CANNOT run, whatever the tuning says.  The launchers refuse on it (GPP_ERR_UNSUPPORTED) and
// tile_is_candidate (conv_igemm.hip) leaves such a tile out; nk = K-steps of the layer (KH * KW * C_in / channels per 128-byte row).

inline bool dual_can_run(const gpp_conv_desc& d, int nk) { return d.C_out >= 384 && d.C_out % 256 == 128 && nk >= 2 && d.split_k <= 1; }

inline bool mix_can_run(const gpp_conv_desc& d, int nk) { return d.C_out % 256 == 0 && nk >= 2 && d.split_k <= 1; }

// 1 x 1, stride 1, one map, pre-split input (and shortcut, of the output's size); whole n-tiles whose count divides the 32 workgroups of an
// XCD; the W n-tile (C_in / 32 K-steps of BN rows) and the four-deep activation ring fit 160 KB of LDS
inline bool ws_can_run(const gpp_conv_desc& d, int bm, int bn)
{
    const gpp_conv_group& G = d.groups[0];
    return (d.x3_split & GPP_X3_IN) && d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad_top == 0 && d.pad_left == 0 && d.n_groups == 1 && d.split_k <= 1 &&
           d.C_out % bn == 0 && 32 % (d.C_out / bn) == 0 && d.C_in % 32 == 0 && G.H_in == G.H_out && G.W_in == G.W_out &&
           (!d.residual || ((d.x3_split & GPP_X3_RES) && G.H_res == G.H_out && G.W_res == G.W_out)) &&
           (d.C_in / 32) * bn * 128 + 4 * bm * 128 <= 160 * 1024;
}

}  // namespace gpp_tiles

#endif  // GPP_CONV_TILES_H_
