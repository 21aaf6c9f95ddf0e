// Smoothing finished tracks offline (include/gpp.h: gpp_track_smooth_f64): the Kalman filter of section 4.34 run
// forward over every segment of an identity, a Rauch-Tung-Striebel pass run backward over what it kept, and a fill row for every frame
// the detector missed inside a segment.  The specification is DESIGN.md's text: every expression there is one statement here, every
// + - * / and sqrt one separately rounded float64 operation (-ffp-contract=off), so that utils/track_smooth.py (NumPy) and
// tests/track_smooth_oracle.py (loops) return the same words.  The row noise, birth covariance, predict, ground rotation and update of
// section 4.34 are csrc/track_kf.h's, the functions csrc/track.hip calls; the ground-only mean steps and the backward step are here.
//
// Two launches.
//   track_smooth_pass   one LANE per segment of two or more cells.  Forward: per cell the predicted and the filtered (x z vx vz, ten
//                       covariance words) = 28 float64 go to the workspace; backward: they come back, and x_s z_s Axx Axz Azz go to the
//                       cell table.  The workspace is laid out for the wavefront, not for the segment: blocks of 64 segments,
//                       [word][cell][lane] with the block's longest segment as pitch, so the 64 lanes at the same step touch 64
//                       consecutive float64.  The entry point orders the segments by length (longest first), so that the lanes of a
//                       wavefront end together and a block's pitch is its first segment's length; no output depends on the order.
//   track_smooth_emit   one THREAD per cell: a detection's row is patched (columns 19 21 25), a gap's fill row is built from its two
//                       detected neighbours, found by walking the segment's cells either way (at most max_gap + 1 of them by the way
//                       the index is made; the loop's bound is the segment).
// No barrier, no LDS, no atomics, no word between workgroups; every loop bound is a function of the index.  In place (rows_out ==
// rows_in) is race-free: the pass has finished before anything is written, and the emit launch reads of other cells' rows only columns
// that no thread writes (every one but 19, 21 and 25).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gpp.h"
#include "track_kf.h"

namespace {

using namespace gpp_kf;                               // kPi, wrap, AXX .. CZZ, kCov and section 4.34's steps

constexpr int kRow = GPP_POSE_COLS;
constexpr int kMaxD = GPP_KITTI_MAX_DETECTIONS;
constexpr int kEgoFields = GPP_TRACK_EGO_FIELDS;
constexpr int kLanes = 64;                           // segments per block of the workspace: one wavefront
constexpr int kWords = 28;                           // per cell: predicted (4 + 10), filtered (4 + 10)
constexpr int kTable = 5;                            // per cell: x_s z_s Axx Axz Azz, laid out [word][cell]
constexpr int kEmitThreads = 256;
static_assert(kWords == 2 * (4 + kCov), "predicted and filtered");

struct state { double x, z, vx, vz, P[kCov]; };
struct m2 { double xx, xz, zx, zz; };                // a general 2 x 2

__device__ __forceinline__ m2 mul(const m2 X, const m2 Y)
{
    return {(X.xx * Y.xx) + (X.xz * Y.zx), (X.xx * Y.xz) + (X.xz * Y.zz), (X.zx * Y.xx) + (X.zz * Y.zx), (X.zx * Y.xz) + (X.zz * Y.zz)};
}
__device__ __forceinline__ m2 tr(const m2 X) { return {X.xx, X.zx, X.xz, X.zz}; }
__device__ __forceinline__ m2 add(const m2 X, const m2 Y) { return {X.xx + Y.xx, X.xz + Y.xz, X.zx + Y.zx, X.zz + Y.zz}; }
__device__ __forceinline__ m2 sub(const m2 X, const m2 Y) { return {X.xx - Y.xx, X.xz - Y.xz, X.zx - Y.zx, X.zz - Y.zz}; }
__device__ __forceinline__ m2 neg(const m2 X) { return {-X.xx, -X.xz, -X.zx, -X.zz}; }
__device__ __forceinline__ m2 sym(double xx, double xz, double zz) { return {xx, xz, xz, zz}; }

// section 4.34, "births": mean (x, z, 0, 0) and born_cov
__device__ __forceinline__ void born(state& s, double x, double z, double rxx, double rxz, double rzz, double speed)
{
    s.x = x; s.z = z; s.vx = 0.0; s.vz = 0.0;
    born_cov(s.P, rxx, rxz, rzz, speed);
}

// section 4.34, "1 predict": x += vx, z += vz; P' = F P F^T + Q
__device__ __forceinline__ void predict(state& s, double q_pos, double q_vel)
{
    s.x = s.x + s.vx;
    s.z = s.z + s.vz;
    predict_cov(s.P, q_pos, q_vel);
}

// section 4.35, the ego step: the mean by the ground part of the record only, the covariance as section 4.34's 1b
__device__ __forceinline__ void ego_step(state& s, const m2 g, double t0, double t2)
{
    const double x = ((g.xx * s.x) + (g.xz * s.z)) + t0, z = ((g.zx * s.x) + (g.zz * s.z)) + t2;
    const double vx = (g.xx * s.vx) + (g.xz * s.vz), vz = (g.zx * s.vx) + (g.zz * s.vz);
    s.x = x; s.z = z; s.vx = vx; s.vz = vz;
    turn_cov(s.P, g.xx, g.xz, g.zx, g.zz);
}

// section 4.35, one backward step: sm holds the smoothed state of cell c + 1 and receives that of cell c; pp is the predicted state of
// cell c + 1, pf the filtered one of cell c, g the ground rotation of the transition into c + 1 (kEgo).  A step whose A or whose Schur
// complement has no determinant > 0 is skipped: the smoothed state of c is its filtered one (J = 0)
template <bool kEgo>
__device__ __forceinline__ void smooth_step(state& sm, const state& pp, const state& pf, const m2 g)
{
    const m2 A = sym(pp.P[AXX], pp.P[AXZ], pp.P[AZZ]), B = {pp.P[BXX], pp.P[BXZ], pp.P[BZX], pp.P[BZZ]};
    const double dA = (A.xx * A.zz) - (A.xz * A.xz);
    const m2 iA = sym(A.zz / dA, -(A.xz / dA), A.xx / dA);
    const m2 W = mul(iA, B);
    const m2 T = mul(tr(B), W);
    const double sxx = pp.P[CXX] - T.xx, sxz = pp.P[CXZ] - T.xz, szz = pp.P[CZZ] - T.zz;
    const double dS = (sxx * szz) - (sxz * sxz);
    if (!(dA > 0.0) || !(dS > 0.0)) {
        sm = pf;
        return;
    }
    const m2 iS = sym(szz / dS, -(sxz / dS), sxx / dS);
    const m2 Fm = neg(mul(W, iS));
    const m2 E = sub(iA, mul(Fm, tr(W)));
    const m2 fA = sym(pf.P[AXX], pf.P[AXZ], pf.P[AZZ]), fB = {pf.P[BXX], pf.P[BXZ], pf.P[BZX], pf.P[BZZ]};
    const m2 fC = sym(pf.P[CXX], pf.P[CXZ], pf.P[CZZ]);
    m2 U1 = add(fA, fB), U2 = fB, U3 = add(tr(fB), fC), U4 = fC;
    if (kEgo) {
        const m2 gt = tr(g);
        U1 = mul(U1, gt); U2 = mul(U2, gt); U3 = mul(U3, gt); U4 = mul(U4, gt);
    }
    const m2 J1 = add(mul(U1, E), mul(U2, tr(Fm))), J2 = add(mul(U1, Fm), mul(U2, iS));
    const m2 J3 = add(mul(U3, E), mul(U4, tr(Fm))), J4 = add(mul(U3, Fm), mul(U4, iS));
    const double dpx = sm.x - pp.x, dpz = sm.z - pp.z, dvx = sm.vx - pp.vx, dvz = sm.vz - pp.vz;
    const m2 DA = sym(sm.P[AXX] - pp.P[AXX], sm.P[AXZ] - pp.P[AXZ], sm.P[AZZ] - pp.P[AZZ]);
    const m2 DB = {sm.P[BXX] - pp.P[BXX], sm.P[BXZ] - pp.P[BXZ], sm.P[BZX] - pp.P[BZX], sm.P[BZZ] - pp.P[BZZ]};
    const m2 DC = sym(sm.P[CXX] - pp.P[CXX], sm.P[CXZ] - pp.P[CXZ], sm.P[CZZ] - pp.P[CZZ]);
    const m2 N1 = add(mul(J1, DA), mul(J2, tr(DB))), N2 = add(mul(J1, DB), mul(J2, DC));
    const m2 N3 = add(mul(J3, DA), mul(J4, tr(DB))), N4 = add(mul(J3, DB), mul(J4, DC));
    const m2 QA = add(mul(N1, tr(J1)), mul(N2, tr(J2))), QB = add(mul(N1, tr(J3)), mul(N2, tr(J4)));
    const m2 QC = add(mul(N3, tr(J3)), mul(N4, tr(J4)));
    sm.x = pf.x + (((J1.xx * dpx) + (J1.xz * dpz)) + ((J2.xx * dvx) + (J2.xz * dvz)));
    sm.z = pf.z + (((J1.zx * dpx) + (J1.zz * dpz)) + ((J2.zx * dvx) + (J2.zz * dvz)));
    sm.vx = pf.vx + (((J3.xx * dpx) + (J3.xz * dpz)) + ((J4.xx * dvx) + (J4.xz * dvz)));
    sm.vz = pf.vz + (((J3.zx * dpx) + (J3.zz * dpz)) + ((J4.zx * dvx) + (J4.zz * dvz)));
    sm.P[AXX] = fA.xx + QA.xx; sm.P[AXZ] = fA.xz + QA.xz; sm.P[AZZ] = fA.zz + QA.zz;
    sm.P[BXX] = fB.xx + QB.xx; sm.P[BXZ] = fB.xz + QB.xz; sm.P[BZX] = fB.zx + QB.zx; sm.P[BZZ] = fB.zz + QB.zz;
    sm.P[CXX] = fC.xx + QC.xx; sm.P[CXZ] = fC.xz + QC.xz; sm.P[CZZ] = fC.zz + QC.zz;
}

// the index as the kernels read it: the entry point's copy behind the workspace
struct index_dev {
    const int64_t* seg_start;    // (n_seg + 1), the caller's order
    const int64_t* block_base;   // (blocks): where the block's words start, in float64
    const int32_t* seg_frame;    // (n_seg)
    const int32_t* order;        // (blocks * 64): the segment of every lane, longest first, -1 for a lane without one
    const int32_t* block_pitch;  // (blocks): the block's longest segment, in cells
    const int32_t* cell_code;    // (cells): the row of a detection, or -(fill + 1) for a gap
    const int32_t* cell_seg;     // (cells)
    const double* ego;           // (N, 16)
    long long cells;
};

__device__ __forceinline__ void store14(double* w, size_t pitch, int first, int c, const state& s)
{
    w[((size_t)(first + 0) * pitch + c) * kLanes] = s.x;
    w[((size_t)(first + 1) * pitch + c) * kLanes] = s.z;
    w[((size_t)(first + 2) * pitch + c) * kLanes] = s.vx;
    w[((size_t)(first + 3) * pitch + c) * kLanes] = s.vz;
#pragma unroll
    for (int k = 0; k < kCov; ++k) w[((size_t)(first + 4 + k) * pitch + c) * kLanes] = s.P[k];
}

__device__ __forceinline__ void load14(const double* w, size_t pitch, int first, int c, state& s)
{
    s.x = w[((size_t)(first + 0) * pitch + c) * kLanes];
    s.z = w[((size_t)(first + 1) * pitch + c) * kLanes];
    s.vx = w[((size_t)(first + 2) * pitch + c) * kLanes];
    s.vz = w[((size_t)(first + 3) * pitch + c) * kLanes];
#pragma unroll
    for (int k = 0; k < kCov; ++k) s.P[k] = w[((size_t)(first + 4 + k) * pitch + c) * kLanes];
}

__device__ __forceinline__ void store_table(double* table, long long cells, long long i, const state& s)
{
    table[0 * cells + i] = s.x;
    table[1 * cells + i] = s.z;
    table[2 * cells + i] = s.P[AXX];
    table[3 * cells + i] = s.P[AXZ];
    table[4 * cells + i] = s.P[AZZ];
}

template <bool kEgo>
__global__ __launch_bounds__(kLanes) void track_smooth_pass(const float* __restrict__ rows, const index_dev ix, const gpp_track_kf_params kf,
                                                            double* __restrict__ words, double* __restrict__ table)
{
    const int lane = threadIdx.x, blk = blockIdx.x;
    const int s = ix.order[(size_t)blk * kLanes + lane];
    if (s < 0) return;
    const long long lo = ix.seg_start[s];
    const int L = (int)(ix.seg_start[s + 1] - lo), frame = ix.seg_frame[s];
    double* w = words + ix.block_base[blk] + lane;
    const size_t pitch = (size_t)ix.block_pitch[blk];

    // forward: cell 0 is a birth from its row
    state cur;
    {
        const float* r = rows + (size_t)ix.cell_code[lo] * kRow;
        const double x = (double)r[19], z = (double)r[21];
        double rxx, rxz, rzz;
        row_noise(x, z, kf, rxx, rxz, rzz);
        born(cur, x, z, rxx, rxz, rzz, kf.birth_speed);
        store14(w, pitch, 14, 0, cur);
    }
    for (int c = 1; c < L; ++c) {
        predict(cur, kf.q_pos, kf.q_vel);
        if (kEgo) {
            const double* e = ix.ego + (size_t)(frame + c) * kEgoFields;
            ego_step(cur, m2{e[0], e[2], e[6], e[8]}, e[9], e[11]);
        }
        state pred = cur;
        const int code = ix.cell_code[lo + c];
        if (code >= 0) {
            const float* r = rows + (size_t)code * kRow;
            const double x = (double)r[19], z = (double)r[21];
            double rxx, rxz, rzz;
            row_noise(x, z, kf, rxx, rxz, rzz);
            if (!update(cur.P, rxx, rxz, rzz, x - cur.x, z - cur.z, cur.x, cur.z, cur.vx, cur.vz)) {
                // a restart: as at a birth from the row.  The step into this cell is skipped on the way back; the predicted covariance
                // is kept as zeros, whose determinant is not > 0: the backward pass needs no flag of its own
                born(cur, x, z, rxx, rxz, rzz, kf.birth_speed);
#pragma unroll
                for (int k = 0; k < kCov; ++k) pred.P[k] = 0.0;
            }
        }
        store14(w, pitch, 0, c, pred);
        store14(w, pitch, 14, c, cur);
    }
    // backward: the last cell's smoothed state is its filtered one
    store_table(table, ix.cells, lo + (L - 1), cur);
    for (int c = L - 2; c >= 0; --c) {
        state pp, pf;
        load14(w, pitch, 0, c + 1, pp);
        load14(w, pitch, 14, c, pf);
        m2 g = {1.0, 0.0, 0.0, 1.0};
        if (kEgo) {
            const double* e = ix.ego + (size_t)(frame + c + 1) * kEgoFields;
            g = m2{e[0], e[2], e[6], e[8]};
        }
        smooth_step<kEgo>(cur, pp, pf, g);
        store_table(table, ix.cells, lo + c, cur);
    }
}

__global__ __launch_bounds__(kEmitThreads) void track_smooth_emit(const float* rows_in, const index_dev ix, const double* __restrict__ table,
                                                                  float* rows_out, double* __restrict__ row_cov,
                                                                  float* __restrict__ fill_rows, double* __restrict__ fill_cov)
{
    const long long i = (long long)blockIdx.x * kEmitThreads + threadIdx.x;
    if (i >= ix.cells) return;
    const int s = ix.cell_seg[i];
    const long long lo = ix.seg_start[s], hi = ix.seg_start[s + 1];
    if (hi - lo < 2) return;                                            // a segment of one cell: its row stays a bit copy
    const double xs = table[0 * ix.cells + i], zs = table[1 * ix.cells + i];
    const double axx = table[2 * ix.cells + i], axz = table[3 * ix.cells + i], azz = table[4 * ix.cells + i];
    const int code = ix.cell_code[i];
    if (code >= 0) {
        const double ry = (double)rows_in[(size_t)code * kRow + 32];
        float* out = rows_out + (size_t)code * kRow;
        out[19] = (float)xs;
        out[21] = (float)zs;
        out[25] = (float)wrap(ry - atan2(xs, zs));
        if (row_cov) {
            row_cov[(size_t)code * 3 + 0] = axx;
            row_cov[(size_t)code * 3 + 1] = axz;
            row_cov[(size_t)code * 3 + 2] = azz;
        }
        return;
    }
    // a gap: the detected neighbours before and behind (the segment's first and last cell are detections: both walks end inside it)
    long long j0 = i - 1, j1 = i + 1;
    while (j0 > lo && ix.cell_code[j0] < 0) --j0;
    while (j1 < hi - 1 && ix.cell_code[j1] < 0) ++j1;
    const float* a = rows_in + (size_t)ix.cell_code[j0] * kRow;
    const float* b = rows_in + (size_t)ix.cell_code[j1] * kRow;
    const double wgt = (double)(i - j0) / (double)(j1 - j0);
    const size_t fill = (size_t)(-(code + 1));
    float* out = fill_rows + fill * kRow;
    const double ra = (double)a[32];
    double delta = wrap((double)b[32] - ra);
    if (delta >= kPi / 2.0) delta -= kPi;
    if (delta < -(kPi / 2.0)) delta += kPi;
    const double ry = wrap(ra + (wgt * delta));
    for (int col = 0; col < kRow; ++col) {
        if (col == 19 || col == 21 || col == 25 || col == 32) continue;      // (never read of another cell's row: see the header)
        const double va = (double)a[col];
        const bool is_code = col == 13 || col == 14 || col >= 33;
        out[col] = is_code ? a[col] : (float)(va + (wgt * ((double)b[col] - va)));
    }
    out[19] = (float)xs;
    out[21] = (float)zs;
    out[25] = (float)wrap(ry - atan2(xs, zs));
    out[32] = (float)ry;
    if (fill_cov) {
        fill_cov[fill * 3 + 0] = axx;
        fill_cov[fill * 3 + 1] = axz;
        fill_cov[fill * 3 + 2] = azz;
    }
}

size_t pad8(size_t n) { return (n + 7) / 8 * 8; }

// the workspace, in bytes: [words][table][ego | seg_start | block_base | seg_frame | order | block_pitch | cell_code | cell_seg]; the part in
// brackets is the index, built on the host in this layout and copied in one piece.  The blocks' words: with the segments ordered by
// length a block's pitch is at most the shortest length of the block before it, so all blocks but the first hold together at most
// `cells` cell columns of 64 lanes, and the first 64 times the longest segment, which has at most min(N, cells) cells (one per frame)
struct layout {
    size_t words, table, ego, seg_start, block_base, seg_frame, order, block_pitch, cell_code, cell_seg, total;
};

layout layout_of(int N, int n_seg, long long cells)
{
    layout l;
    const size_t blocks = ((size_t)n_seg + kLanes - 1) / kLanes;
    const size_t longest = (size_t)std::min<long long>(N, cells);
    size_t at = 0;
    l.words = at; at += (size_t)kWords * ((size_t)cells + kLanes * longest) * sizeof(double);
    l.table = at; at += (size_t)kTable * (size_t)cells * sizeof(double);
    l.ego = at; at += (size_t)N * kEgoFields * sizeof(double);
    l.seg_start = at; at += ((size_t)n_seg + 1) * sizeof(int64_t);
    l.block_base = at; at += blocks * sizeof(int64_t);
    l.seg_frame = at; at += pad8((size_t)n_seg * sizeof(int32_t));
    l.order = at; at += pad8(blocks * kLanes * sizeof(int32_t));
    l.block_pitch = at; at += pad8(blocks * sizeof(int32_t));
    l.cell_code = at; at += pad8((size_t)cells * sizeof(int32_t));
    l.cell_seg = at; at += pad8((size_t)cells * sizeof(int32_t));
    l.total = at;
    return l;
}

}  // namespace

extern "C" int gpp_track_smooth_workspace_bytes(int N, int n_seg, long long cells, size_t* bytes)
{
    if (N < 0 || n_seg < 0 || cells < 0 || !bytes) return GPP_ERR_BAD_ARG;
    *bytes = layout_of(N, n_seg, cells).total;
    return GPP_OK;
}

extern "C" int gpp_track_smooth_f64(const float* rows_in, int N, int D, const int64_t* seg_start, const int32_t* seg_frame,
                                    const int32_t* cell_row, int n_seg, const gpp_track_kf_params* kf, const double* ego, float* rows_out,
                                    double* row_cov, float* fill_rows, double* fill_cov, void* workspace, size_t workspace_bytes,
                                    void* stream)
{
    // the checks of the contract, all of them on the host and before anything is launched or written
    if (N < 0 || D < 0 || n_seg < 0 || D > kMaxD || !kf || !seg_start) return GPP_ERR_BAD_ARG;
    const long long rows_total = (long long)N * (long long)D;
    if (rows_total > 0x7fffffffLL) return GPP_ERR_BAD_ARG;
    if (gpp_kf::kf_params_bad(*kf)) return GPP_ERR_BAD_ARG;
    if (seg_start[0] != 0) return GPP_ERR_BAD_ARG;
    for (int s = 0; s < n_seg; ++s)
        if (seg_start[s + 1] <= seg_start[s]) return GPP_ERR_BAD_ARG;
    const long long cells = seg_start[n_seg];
    if (cells > 0 && (!seg_frame || !cell_row || rows_total == 0)) return GPP_ERR_BAD_ARG;
    if (rows_total > 0 && (!rows_in || !rows_out)) return GPP_ERR_BAD_ARG;
    long long fills = 0;
    {
        std::vector<uint8_t> seen(cells > 0 ? (size_t)(rows_total + 7) / 8 : 0, 0);
        for (int s = 0; s < n_seg; ++s) {
            const long long lo = seg_start[s], len = seg_start[s + 1] - lo;
            if (seg_frame[s] < 0 || (long long)seg_frame[s] + len > N) return GPP_ERR_BAD_ARG;
            if (cell_row[lo] < 0 || cell_row[lo + len - 1] < 0) return GPP_ERR_BAD_ARG;
            for (long long c = 0; c < len; ++c) {
                const int32_t r = cell_row[lo + c];
                if (r == -1) { ++fills; continue; }
                if (r < 0 || r >= rows_total || r / D != seg_frame[s] + c) return GPP_ERR_BAD_ARG;
                if (seen[(size_t)r >> 3] & (1u << (r & 7))) return GPP_ERR_BAD_ARG;
                seen[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7));
            }
        }
    }
    if (ego)
        for (int f = 0; f < N; ++f)
            if (gpp_kf::ego_record_bad(ego + (size_t)f * kEgoFields)) return GPP_ERR_BAD_ARG;
    if (fills > 0 && !fill_rows) return GPP_ERR_BAD_ARG;
    if (cells > 0 && !workspace) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)rows_in | (uintptr_t)rows_out | (uintptr_t)fill_rows) & 3u) return GPP_ERR_ALIGN;
    if (((uintptr_t)row_cov | (uintptr_t)fill_cov | (uintptr_t)workspace) & 7u) return GPP_ERR_ALIGN;
    const layout l = layout_of(N, n_seg, cells);
    if (cells > 0 && workspace_bytes < l.total) return GPP_ERR_WORKSPACE;

    hipStream_t q = (hipStream_t)stream;
    hipError_t e;
    if (rows_total > 0 && rows_out != rows_in) {
        e = hipMemcpyAsync(rows_out, rows_in, (size_t)rows_total * kRow * sizeof(float), hipMemcpyDeviceToDevice, q);
        if (e != hipSuccess) return (int)e;
    }
    if (rows_total > 0 && row_cov) {
        e = hipMemsetAsync(row_cov, 0, (size_t)rows_total * 3 * sizeof(double), q);
        if (e != hipSuccess) return (int)e;
    }
    if (cells == 0) return GPP_OK;

    // the lanes: the segments of two or more cells, longest first (a stable order: equal lengths keep the caller's)
    std::vector<int32_t> lanes;
    lanes.reserve((size_t)n_seg);
    for (int s = 0; s < n_seg; ++s)
        if (seg_start[s + 1] - seg_start[s] >= 2) lanes.push_back(s);
    if (lanes.empty()) return GPP_OK;                                   // (nothing is smoothed, and a gap needs three cells)
    std::stable_sort(lanes.begin(), lanes.end(), [&](int32_t a, int32_t b) {
        return seg_start[a + 1] - seg_start[a] > seg_start[b + 1] - seg_start[b];
    });
    const size_t blocks = (lanes.size() + kLanes - 1) / kLanes;

    // the index in the workspace's layout, from l.ego on, in one host buffer and one copy
    std::vector<uint64_t> host((l.total - l.ego) / 8, 0);
    char* base = (char*)host.data() - l.ego;
    if (ego) memcpy(base + l.ego, ego, (size_t)N * kEgoFields * sizeof(double));
    memcpy(base + l.seg_start, seg_start, ((size_t)n_seg + 1) * sizeof(int64_t));
    memcpy(base + l.seg_frame, seg_frame, (size_t)n_seg * sizeof(int32_t));
    int64_t* h_base = (int64_t*)(base + l.block_base);
    int32_t* h_order = (int32_t*)(base + l.order);
    int32_t* h_pitch = (int32_t*)(base + l.block_pitch);
    int32_t* h_code = (int32_t*)(base + l.cell_code);
    int32_t* h_seg = (int32_t*)(base + l.cell_seg);
    size_t at = 0;
    for (size_t b = 0; b < blocks; ++b) {
        const int32_t first = lanes[b * kLanes];
        h_pitch[b] = (int32_t)(seg_start[first + 1] - seg_start[first]);
        h_base[b] = (int64_t)at;
        at += (size_t)kWords * (size_t)h_pitch[b] * kLanes;
        for (int k = 0; k < kLanes; ++k) {
            const size_t t = b * kLanes + k;
            h_order[t] = t < lanes.size() ? lanes[t] : -1;
        }
    }
    if (at * sizeof(double) > l.table - l.words) return GPP_ERR_WORKSPACE;          // (cannot happen: the bound of layout_of)
    long long fill = 0;
    for (int s = 0; s < n_seg; ++s)
        for (long long i = seg_start[s]; i < seg_start[s + 1]; ++i) {
            h_seg[i] = s;
            h_code[i] = cell_row[i] >= 0 ? cell_row[i] : (int32_t)(-(fill++) - 1);
        }
    char* dev = (char*)workspace;
    // (a copy the host waits for: the buffer above is gone when this function returns; it is ordered on the stream like the launches)
    e = hipMemcpyWithStream(dev + l.ego, base + l.ego, l.total - l.ego, hipMemcpyHostToDevice, q);
    if (e != hipSuccess) return (int)e;

    index_dev ix;
    ix.seg_start = (const int64_t*)(dev + l.seg_start);
    ix.block_base = (const int64_t*)(dev + l.block_base);
    ix.seg_frame = (const int32_t*)(dev + l.seg_frame);
    ix.order = (const int32_t*)(dev + l.order);
    ix.block_pitch = (const int32_t*)(dev + l.block_pitch);
    ix.cell_code = (const int32_t*)(dev + l.cell_code);
    ix.cell_seg = (const int32_t*)(dev + l.cell_seg);
    ix.ego = (const double*)(dev + l.ego);
    ix.cells = cells;
    double* words = (double*)(dev + l.words);
    double* table = (double*)(dev + l.table);
    if (ego) track_smooth_pass<true><<<dim3((unsigned)blocks), dim3(kLanes), 0, q>>>(rows_in, ix, *kf, words, table);
    else track_smooth_pass<false><<<dim3((unsigned)blocks), dim3(kLanes), 0, q>>>(rows_in, ix, *kf, words, table);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const unsigned grid = (unsigned)((cells + kEmitThreads - 1) / kEmitThreads);
    track_smooth_emit<<<dim3(grid), dim3(kEmitThreads), 0, q>>>(rows_in, ix, table, rows_out, row_cov, fill_rows, fill_cov);
    e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
