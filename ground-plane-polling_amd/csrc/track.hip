// Tracking of cuboids across frames on gfx950 (MI355X): the rows of gpp_pose_f32 of one frame are associated greedily with the cuboids
// carried over from the frames before, and every carried cuboid is a fixed-gain (alpha-beta) filter.  DESIGN.md section 4.28 is the
// specification, utils/track.py the host form, tests/track_oracle.py the loop-written oracle; include/gpp.h has the contract.
//
//   track_kernel   one workgroup of 128 threads per sequence; the state of the sequence lives in LDS for the whole call and the frames
//                  are walked in order.  Thread t is slot t and row t.  Per frame, with a barrier between the phases:
//     1  one thread per row: liveness, blindness, the fields and (BEV / 3-D) the placed corners into LDS -- every input byte the step
//        needs is read here, before anything of the frame is written: rows_out may be rows_in; one thread per slot: the prediction and
//        the predicted corners; the frame's candidate table (workspace) is set to "no candidate"
//     2  the occupied slots and the live, non-blind rows are listed in ascending order (ballot + prefix)
//     3  the listed slots x the listed rows over the lanes.  DIST: q against threshold^2.  BEV / 3-D: the lanes first gate 4096 pairs and
//        list the survivors in LDS, then clip the list together with every lane busy (cuboid_nms.hip).  A candidate's key -- q, or minus
//        the overlap: the smaller the better -- goes into the table
//     4  the greedy assignment, several candidates per round: every open slot keeps the best free row of its table line (ties: the
//        smaller row), every free row the best open slot of its column (ties: the smaller slot); a pair that names each other is
//        taken -- nothing before it in the order (key, slot, row) shares its slot or row, so the serial rule takes it as well, and the
//        best candidate left is always such a pair.  A thread looks again only when its partner has gone.  At most min(slots, rows)
//        rounds (a scene of separate cars needs one); every thread sees the same rounds
//     5  update of the matched slots, deaths; then the births in ascending row order into the free slots in ascending slot order
//        (ballot + prefix on both sides)
//     6  one thread per row: ids, hits and the row
//
// The table: T x D reaches 16 384 float64, 128 KiB -- it does not fit into LDS beside the 32 KiB of clipping buffers, so it lies in a
// workspace in HBM (one per sequence; a workgroup only ever reads what it wrote itself behind a barrier), once as [slot][row] and once
// as [row][slot], so that both walks of phase 4 are coalesced.  Keeping "only the candidates"
// has no bound below T x D either: with DIST and a wide threshold every pair is one.
//
// Every loop bound is a function of D, the slot count and the frame count; there is no spin wait and no word passes between workgroups;
// every barrier is reached by all 128 threads (the conditions around them are uniform: they come from LDS words written before the last
// barrier, or from kernel arguments).
//
// Arithmetic: float64, every operation separate (this file is compiled with -ffp-contract=off), as cuboid_nms.hip.
//
//   track_kernel<true>   gpp_track_optimal_f64: the same kernel with another phase 4 -- the optimal one-to-one
//                  assignment of the frame.  Phases 1, 2, 5 and 6 are the statements above.  Behind phase 2 all 128 threads fill an n x n
//                  int32 matrix in LDS (n = max(slots, rows) listed, stride n) with 2^20; phase 3 writes a candidate's integer cell at
//                  (a, c), its place in the two lists, instead of its key into the table; in phase 4 wavefront 0 runs
//                  gpp_mot::assign_rows (csrc/mot_assign.h, section 4.29's routine) on it while wavefront 1 waits at the barrier, and lane
//                  l then writes the matches of its columns l and l + 64: a column's row is a match iff their cell is below 2^20.
//                  The matrix is 64 KiB beside the 81 KiB of the greedy form: 145 KiB of the 160 KiB a workgroup may have, so it is
//                  declared on its own and overlays nothing.  There is no table in HBM in this form: the workspace holds seq_start only.
//                  The greedy instantiation has none of these statements (if constexpr) and no matrix.
//
//   track_kernel<*, true>   gpp_track_ego_f64: either kernel with step 1b between the prediction and the
//                  predicted corners -- the slot's thread carries its position, its velocity and r_y into the frame's camera coordinates
//                  by the frame's ego record.  The entry point has checked the records on the host and copied them into the workspace
//                  behind everything else; every thread takes the frame's 13 words from there (the address is uniform) and a slot's
//                  thread uses them.  No barrier, no loop and no LDS word more; the <*, false> instantiations have none of it.
//
//   track_kernel<*, *, true>   gpp_track_kf_f64: any of the four with a Kalman filter on (x, z, vx, vz) of every
//                  slot.  Thread t keeps the ten covariance words of slot t in registers from the call's first frame to its last (cov_in
//                  is read and cov_out written by the slot's own thread only: the two may be one buffer).  LDS holds what phases 3 and 5
//                  read of OTHER threads: the predicted A of every slot (3 KiB) and the noise R of every row (3 KiB), declared on their
//                  own beside everything else -- 89 536 bytes declared in the greedy forms (83 392 without the filter), 154 784 of
//                  163 840 in the optimal ones (148 640 without); none of the four uses scratch (193 - 195 VGPRs against 169).  A birth is
//                  written by the row's thread, the covariance lives with the slot's: the row leaves its number in s_mrow[slot] (idle
//                  behind phase 5) and the slot's thread takes R from there behind the barrier the births end with.  No barrier more
//                  than before, and none inside a divergent branch; no loop more.  kEgo here means "records were given".  The
//                  <*, *, false> instantiations have none of it (if constexpr).  The filter's expressions -- row noise, birth covariance,
//                  predict, the ground rotation, the update -- are csrc/track_kf.h's, shared with csrc/track_smooth.hip; here stay the
//                  Mahalanobis key of phase 3 and the 3-D mean of step 1b.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "gpp.h"
#include "mot_assign.h"
#include "rot_iou.h"
#include "track_kf.h"

namespace {

using namespace gpp_kf;                               // kPi, wrap, AXX .. CZZ, kCov and section 4.34's steps

constexpr int kMaxD = GPP_KITTI_MAX_DETECTIONS;
constexpr int kSlots = GPP_TRACK_MAX_TRACKS;
constexpr int kRow = GPP_POSE_COLS;
constexpr int kThreads = 128;
constexpr double kGateSlack = 1.0634765625;          // (1 + 1/32)^2, the gate of cuboid_nms.hip
constexpr int kChunk = 4096;                         // pairs gated per round
constexpr size_t kSeqBytes = 256;                    // the workspace starts with seq_start's copy, padded to a multiple of this
constexpr int32_t kScale = 1 << GPP_MOT_SCALE_BITS;  // section 4.32: the cell of a pair that is no candidate, and of padding
constexpr int kSide = kSlots > kMaxD ? kSlots : kMaxD;                 // the largest matrix of section 4.32
constexpr int kEgoFields = GPP_TRACK_EGO_FIELDS;     // section 4.33: R row-major (9), t (3), dyaw (1), three words that are 0

static_assert(kThreads == kSlots && kThreads >= kMaxD, "one thread per slot and per row");
static_assert(kChunk <= 65536, "a pair's offset into its chunk is 16 bits");
static_assert(sizeof(gpp_track_state) % 8 == 0, "states are laid out back to back");
static_assert(kSide <= 2 * gpp_mot::kWave, "assign_rows: a lane owns two columns");

enum { FX = 0, FY, FZ, FRY, FH, FW, FL, FVX, FVY, FVZ };
static_assert(sizeof(gpp_track_cov) == (size_t)kCov * kSlots * sizeof(double), "field-major, back to back");

// section 4.34, what the Kalman instantiations take beyond the others
struct kf_args {
    const gpp_track_cov* cov_in;
    gpp_track_cov* cov_out;
    gpp_track_kf_params p;
};

// the number of threads below `tid` whose flag is set, and the number of all; two barriers, reached by everyone
__device__ __forceinline__ int block_rank(bool flag, int tid, int* s_wave, int& total)
{
    const unsigned long long m = __ballot(flag);
    const int lane = tid & 63, w = tid >> 6;
    if (lane == 0) s_wave[w] = __popcll(m);
    __syncthreads();
    const int before = __popcll(m & ((1ull << lane) - 1ull)) + (w ? s_wave[0] : 0);
    total = s_wave[0] + s_wave[1];
    __syncthreads();
    return before;
}

size_t seq_bytes(int S) { return ((size_t)(S + 1) * sizeof(int32_t) + kSeqBytes - 1) / kSeqBytes * kSeqBytes; }
size_t plain_bytes(int S) { return seq_bytes(S) + (size_t)S * 2 * kSlots * kMaxD * sizeof(double); }     // gpp_track_workspace_bytes

template <bool kOptimal, bool kEgo, bool kKf>
__global__ __launch_bounds__(kThreads) void track_kernel(const float* rows_in, int N, int D, const int32_t* __restrict__ seq_start,
                                                         const gpp_track_state* states_in, gpp_track_state* states_out,
                                                         gpp_track_params prm, float* rows_out, int32_t* track_ids, int32_t* track_hits,
                                                         double* tables, const double* __restrict__ ego, kf_args kfa)
{
    __shared__ double s_x[2][rot_iou::kMaxVerts][kThreads];
    __shared__ double s_z[2][rot_iou::kMaxVerts][kThreads];
    __shared__ gpp_track_state st;
    __shared__ double r_f[7][kMaxD];                     // the row's x y z r_y h w l (the order of the state's fields)
    __shared__ double r_cx[4][kMaxD], r_cz[4][kMaxD], r_rad[kMaxD], r_area[kMaxD];
    __shared__ double t_cx[4][kSlots], t_cz[4][kSlots], t_rad[kSlots], t_area[kSlots];
    __shared__ float r_score[kMaxD];
    __shared__ int16_t s_tlist[kSlots], s_rlist[kMaxD], s_free[kSlots], s_bt[kMaxD];     // s_bt: phase 4, the row's best open slot
    __shared__ int16_t s_mrow[kSlots], s_mslot[kMaxD];   // the slot's row and the row's slot, -1: none
    __shared__ int16_t r_slot[kMaxD];                    // phase 5: the slot a row ends in (matched or born), -1: none
    __shared__ unsigned char r_flag[kMaxD];              // 1 live, 2 blind
    __shared__ uint16_t s_pairs[kChunk];
    __shared__ unsigned long long s_closed[2], s_gone[2];             // phase 4: the slots taken this round, the rows taken so far
    __shared__ int s_wave[2], s_listed;
    int32_t* s_cost = nullptr;                           // section 4.32: the frame's n x n matrix, stride n
    if constexpr (kOptimal) {
        __shared__ int32_t s_matrix[kSide * kSide];
        s_cost = s_matrix;
    }
    double (*s_A)[kSlots] = nullptr;                     // section 4.34: the predicted Axx Axz Azz of every slot ...
    double (*s_R)[kMaxD] = nullptr;                      // ... and Rxx Rxz Rzz of every live, non-blind row
    if constexpr (kKf) {
        __shared__ double s_cov_a[3][kSlots];
        __shared__ double s_noise[3][kMaxD];
        s_A = s_cov_a;
        s_R = s_noise;
    }

    const int seq = blockIdx.x, tid = threadIdx.x;
    int f0 = seq_start[seq], f1 = seq_start[seq + 1];
    f0 = f0 < 0 ? 0 : f0;                                // (the host has checked the ranges; no frame index leaves [0, N) whatever arrives)
    f1 = f1 > N ? N : f1;
    double* tab = nullptr;                                           // [slot][row]: a row's thread walks its column, coalesced over the rows
    double* tab_dt = nullptr;                                        // [row][slot], the same keys: a slot's thread walks its line, coalesced
    if constexpr (!kOptimal) {
        tab = tables + (size_t)seq * 2 * kSlots * kMaxD;
        tab_dt = tab + kSlots * kMaxD;
    }
    bool iou = prm.metric != GPP_TRACK_DIST;
    bool maha = false;
    if constexpr (kKf) {
        maha = prm.metric == GPP_TRACK_MAHA;
        iou = iou && !maha;
    }
    const double thr2 = prm.threshold * prm.threshold;
    double P[kCov];                                      // (Kalman) the slot's covariance, here for the whole call
    if constexpr (kKf) {
#pragma unroll
        for (int k = 0; k < kCov; ++k) P[k] = kfa.cov_in[seq].p[k][tid];
    }

    // ---- the state into LDS, all of it before anything is written: states_out may be states_in
    {
        const uint32_t* from = (const uint32_t*)(states_in + seq);
        uint32_t* to = (uint32_t*)&st;
        for (int k = tid; k < (int)(sizeof(gpp_track_state) / 4); k += kThreads) to[k] = from[k];
    }
    __syncthreads();

    for (int f = f0; f < f1; ++f) {
        const float* src = rows_in + (size_t)f * D * kRow;
        float* dst = rows_out + (size_t)f * D * kRow;

        // ---- 1: rows, predictions, the empty table
        {
            unsigned char flag = 0;
            if (tid < D) {
                const float* r = src + (size_t)tid * kRow;
                if (r[14] >= 0.0f) {
                    flag = 1;
                    const double x = (double)r[19], y = (double)r[31], z = (double)r[21], ry = (double)r[32];
                    const double h = (double)r[30], w = (double)r[17], l = (double)r[18];
                    if (isnan(x) || isnan(y) || isnan(z) || isnan(ry) || isnan(h) || isnan(w) || isnan(l)) flag |= 2;
                    r_f[FX][tid] = x; r_f[FY][tid] = y; r_f[FZ][tid] = z; r_f[FRY][tid] = ry;
                    r_f[FH][tid] = h; r_f[FW][tid] = w; r_f[FL][tid] = l;
                    r_score[tid] = r[12];
                    if (iou && !(flag & 2)) {
                        const double c = cos(ry), s = sin(ry), hl = l / 2.0, hw = w / 2.0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) rot_iou::corner(k, c, s, hl, hw, x, z, r_cx[k][tid], r_cz[k][tid]);
                        r_rad[tid] = sqrt(hl * hl + hw * hw);
                        r_area[tid] = l * w;
                    }
                    if constexpr (kKf) {
                        if (!(flag & 2)) {               // the row's noise: along and across its viewing ray
                            double rxx, rxz, rzz;
                            row_noise(x, z, kfa.p, rxx, rxz, rzz);
                            s_R[0][tid] = rxx; s_R[1][tid] = rxz; s_R[2][tid] = rzz;
                        }
                    }
                }
            }
            r_flag[tid] = flag;
            s_mslot[tid] = -1;
            r_slot[tid] = -1;
            s_mrow[tid] = -1;
            double e[13];                                // (ego) the frame's record: R row-major, t, dyaw
            if constexpr (kEgo) {
#pragma unroll
                for (int k = 0; k < 13; ++k) e[k] = ego[(size_t)f * kEgoFields + k];
            }
            if (st.id1[tid] != 0) {
                double x = st.box[FX][tid] + st.box[FVX][tid];
                double y = st.box[FY][tid] + st.box[FVY][tid];
                double z = st.box[FZ][tid] + st.box[FVZ][tid];
                if constexpr (kEgo) {                    // 1b: into this frame's camera coordinates, all from the predicted x y z
                    const double px = x, py = y, pz = z;
                    const double vx = st.box[FVX][tid], vy = st.box[FVY][tid], vz = st.box[FVZ][tid];
                    x = ((e[0] * px + e[1] * py) + e[2] * pz) + e[9];
                    y = ((e[3] * px + e[4] * py) + e[5] * pz) + e[10];
                    z = ((e[6] * px + e[7] * py) + e[8] * pz) + e[11];
                    st.box[FVX][tid] = (e[0] * vx + e[1] * vy) + e[2] * vz;
                    st.box[FVY][tid] = (e[3] * vx + e[4] * vy) + e[5] * vz;
                    st.box[FVZ][tid] = (e[6] * vx + e[7] * vy) + e[8] * vz;
                    st.box[FRY][tid] = wrap(st.box[FRY][tid] + e[12]);
                }
                st.box[FX][tid] = x; st.box[FY][tid] = y; st.box[FZ][tid] = z;
                if constexpr (kKf) {                     // 1: P = F P F^T + Q, all from the old values
                    predict_cov(P, kfa.p.q_pos, kfa.p.q_vel);
                    if constexpr (kEgo) turn_cov(P, e[0], e[2], e[6], e[8]);     // 1b: the ground part of the record's rotation
                    s_A[0][tid] = P[AXX]; s_A[1][tid] = P[AXZ]; s_A[2][tid] = P[AZZ];
                }
                if (iou) {
                    const double ry = st.box[FRY][tid], l = st.box[FL][tid], w = st.box[FW][tid];
                    const double c = cos(ry), s = sin(ry), hl = l / 2.0, hw = w / 2.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) rot_iou::corner(k, c, s, hl, hw, x, z, t_cx[k][tid], t_cz[k][tid]);
                    t_rad[tid] = sqrt(hl * hl + hw * hw);
                    t_area[tid] = l * w;
                }
            }
            if constexpr (!kOptimal) {
                if (tid < D)                             // (id1 changes in phase 5 only: every thread sees the same slots here)
                    for (int t = 0; t < kSlots; ++t)
                        if (st.id1[t] != 0) tab[t * kMaxD + tid] = INFINITY;
                if (st.id1[tid] != 0)
                    for (int d = 0; d < D; ++d) tab_dt[d * kSlots + tid] = INFINITY;
            }
        }
        __syncthreads();

        // ---- 2: the lists
        int nT, nR;
        {
            const bool occupied = st.id1[tid] != 0, valid = r_flag[tid] == 1;
            const int a = block_rank(occupied, tid, s_wave, nT);
            if (occupied) s_tlist[a] = (int16_t)tid;
            const int c = block_rank(valid, tid, s_wave, nR);
            if (valid) s_rlist[c] = (int16_t)tid;
        }
        __syncthreads();

        // ---- (optimal) the matrix, all of it "no candidate": n, nT and nR are the same in every thread, n = 0 takes the barrier too
        int n = 0;
        if constexpr (kOptimal) {
            n = nT > nR ? nT : nR;
            for (int k = tid; k < n * n; k += kThreads) s_cost[k] = kScale;
            __syncthreads();
        }

        // ---- 3: the candidates.  Pair p = a * nR + c: slot tlist[a], row rlist[c]
        const int pairs = nT * nR;
        if (!iou) {
            for (int p = tid; p < pairs; p += kThreads) {
                const int t = s_tlist[p / nR], d = s_rlist[p % nR];
                const double dx = r_f[FX][d] - st.box[FX][t], dz = r_f[FZ][d] - st.box[FZ][t];
                double q = dx * dx + dz * dz;
                bool cand = q < thr2;
                if constexpr (kKf) {
                    if (maha) {                          // q is the squared Mahalanobis distance under S = A + R
                        const double sxx = s_A[0][t] + s_R[0][d], sxz = s_A[1][t] + s_R[1][d], szz = s_A[2][t] + s_R[2][d];
                        const double det = (sxx * szz) - (sxz * sxz);
                        q = ((((szz * dx) * dx) - ((2.0 * (sxz * dx)) * dz)) + ((sxx * dz) * dz)) / det;
                        cand = det > 0.0 && q < thr2;
                    }
                }
                if (cand) {
                    if constexpr (kOptimal) {
                        const double r = q / thr2;
                        const double x = r * 1048576.0;
                        const double cell = floor(x);
                        s_cost[(p / nR) * n + p % nR] = cell < (double)(kScale - 1) ? (int32_t)cell : kScale - 1;
                    } else {
                        tab[t * kMaxD + d] = q; tab_dt[d * kSlots + t] = q;
                    }
                }
            }
        } else {
            for (int base = 0; base < pairs; base += kChunk) {
                if (tid == 0) s_listed = 0;
                __syncthreads();
                const int end = base + kChunk < pairs ? base + kChunk : pairs;
                for (int p = base + tid; p < end; p += kThreads) {
                    const int t = s_tlist[p / nR], d = s_rlist[p % nR];
                    // the gate: an empty intersection is an overlap of 0 (or 0 / 0), which is above no threshold >= 0
                    const double ddx = st.box[FX][t] - r_f[FX][d], ddz = st.box[FZ][t] - r_f[FZ][d], reach = t_rad[t] + r_rad[d];
                    if (ddx * ddx + ddz * ddz > reach * reach * kGateSlack) continue;
                    s_pairs[atomicAdd(&s_listed, 1)] = (uint16_t)(p - base);       // (at most kChunk pairs are looked at per chunk)
                }
                __syncthreads();
                const int listed = s_listed;
                for (int q = tid; q < listed; q += kThreads) {
                    const int p = base + s_pairs[q];
                    const int t = s_tlist[p / nR], d = s_rlist[p % nR];
                    double gX[4], gZ[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        gX[k] = r_cx[k][d]; gZ[k] = r_cz[k][d];
                        s_x[0][k][tid] = t_cx[k][t]; s_z[0][k][tid] = t_cz[k][t];
                    }
                    const double inter = rot_iou::intersection<kThreads>(s_x, s_z, tid, gX, gZ);
                    const double area_d = t_area[t], area_g = r_area[d];
                    double o;
                    if (prm.metric == GPP_TRACK_BEV) {
                        o = inter / (area_d + area_g - inter);
                    } else {
                        const double dh = st.box[FH][t], gh = r_f[FH][d];
                        const double hh = rot_iou::height_overlap(st.box[FY][t], dh, r_f[FY][d], gh);
                        const double iv = inter * hh;
                        const double vol_d = area_d * dh, vol_g = area_g * gh;
                        o = iv / (vol_d + vol_g - iv);
                    }
                    if (o > prm.threshold) {
                        if constexpr (kOptimal) {
                            const double scaled = o * 1048576.0;
                            const int32_t cell = kScale - (int32_t)floor(scaled < 1048576.0 ? scaled : 1048576.0);
                            s_cost[(p / nR) * n + p % nR] = cell < kScale - 1 ? cell : kScale - 1;
                        } else {
                            tab[t * kMaxD + d] = -o; tab_dt[d * kSlots + t] = -o;
                        }
                    }
                }
                __syncthreads();
            }
        }
        __syncthreads();

        // ---- 4: the greedy assignment, several candidates per round.  A pair is taken when the row is the best free row of the slot (ties:
        // the smaller row) AND the slot is the best open slot of the row (ties: the smaller slot): no candidate before it in the order
        // (key, slot, row) shares its slot or its row with it, so the serial rule takes it too; the best candidate of all that are left
        // is always such a pair, so every round takes at least one.  A thread keeps what it found until its partner has gone
        if constexpr (kOptimal) {
            // ---- 4 (optimal): one wavefront on the matrix, the other waits at the barrier below.  Lane l holds the matrix rows of its
            // columns l and l + 64; a column below nR whose row's cell is below 2^20 is a match (padding and non-candidates hold 2^20).
            // Without slots or without rows every cell is 2^20 and nothing can match: such a frame (the first of every sequence) is
            // not walked
            if (tid < gpp_mot::kWave && pairs > 0) {
                int p[2];
                gpp_mot::assign_rows(s_cost, n, tid, p);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int c = tid + gpp_mot::kWave * s;
                    if (c < nR && s_cost[p[s] * n + c] < kScale) {
                        const int t = s_tlist[p[s]], d = s_rlist[c];
                        s_mrow[t] = (int16_t)d;
                        s_mslot[d] = (int16_t)t;
                    }
                }
            }
        } else {
            const bool is_slot = st.id1[tid] != 0, is_row = r_flag[tid] == 1;
            bool open = is_slot, unmatched = is_row, scan_line = is_slot, scan_column = is_row;
            unsigned long long free_lo = ~0ull, free_hi = ~0ull;     // the free rows and the open slots, kept by every thread alike
            unsigned long long open_lo = ~0ull, open_hi = ~0ull;
            int bd = -1, bt = -1;
            const int rounds = nT < nR ? nT : nR;
            for (int round = 0; round < rounds; ++round) {
                if (open && scan_line) {                 // the slot's line, by rows: coalesced over the slots
                    double bkey = INFINITY;
                    bd = -1;
#pragma unroll 4
                    for (int c = 0; c < nR; ++c) {
                        const int d = s_rlist[c];
                        const bool is_free = ((d < 64 ? free_lo >> d : free_hi >> (d - 64)) & 1ull) != 0ull;
                        const double key = tab_dt[d * kSlots + tid];
                        if (is_free && key < bkey) { bkey = key; bd = d; }       // (strict: of equal keys the smaller row stays)
                    }
                    scan_line = false;
                }
                if (unmatched && scan_column) {          // the row's column, by slots: coalesced over the rows
                    double bkey = INFINITY;
                    bt = -1;
#pragma unroll 4
                    for (int a = 0; a < nT; ++a) {
                        const int t = s_tlist[a];
                        const bool is_open = ((t < 64 ? open_lo >> t : open_hi >> (t - 64)) & 1ull) != 0ull;
                        const double key = tab[t * kMaxD + tid];
                        if (is_open && key < bkey) { bkey = key; bt = t; }       // (strict: of equal keys the smaller slot stays)
                    }
                    scan_column = false;
                }
                s_bt[tid] = (int16_t)(unmatched ? bt : -1);
                __syncthreads();
                const bool take = open && bd >= 0 && s_bt[bd] == tid;
                if (take) {
                    open = false;
                    s_mrow[tid] = (int16_t)bd;
                    s_mslot[bd] = (int16_t)tid;
                }
                const unsigned long long closed = __ballot(take);
                if ((tid & 63) == 0) s_closed[tid >> 6] = closed;
                __syncthreads();
                if (unmatched && s_mslot[tid] >= 0) unmatched = false;
                const unsigned long long gone = __ballot(is_row && !unmatched);
                if ((tid & 63) == 0) s_gone[tid >> 6] = gone;
                const unsigned long long closed_lo = s_closed[0], closed_hi = s_closed[1];
                __syncthreads();
                if ((closed_lo | closed_hi) == 0ull) break;          // (the same for every thread: no candidate is left)
                open_lo &= ~closed_lo; open_hi &= ~closed_hi;
                free_lo = ~s_gone[0]; free_hi = ~s_gone[1];
                if (open && bd >= 0 && !((bd < 64 ? free_lo >> bd : free_hi >> (bd - 64)) & 1ull)) scan_line = true;
                if (unmatched && bt >= 0 && !((bt < 64 ? open_lo >> bt : open_hi >> (bt - 64)) & 1ull)) scan_column = true;
            }
        }
        __syncthreads();

        // ---- 5: update and deaths (one thread per slot) ...
        if (st.id1[tid] != 0) {
            const int d = s_mrow[tid];
            if (d >= 0) {
                bool kalman = false;
                if constexpr (kKf) {
                    const double rxx = s_R[0][d], rxz = s_R[1][d], rzz = s_R[2][d];
                    double x = st.box[FX][tid], z = st.box[FZ][tid], vx = st.box[FVX][tid], vz = st.box[FVZ][tid];
                    kalman = update(P, rxx, rxz, rzz, r_f[FX][d] - x, r_f[FZ][d] - z, x, z, vx, vz);
                    if (kalman) {
                        st.box[FX][tid] = x; st.box[FZ][tid] = z; st.box[FVX][tid] = vx; st.box[FVZ][tid] = vz;
                    } else {
                        born_cov(P, rxx, rxz, rzz, kfa.p.birth_speed);     // the fixed gains below, P as at birth
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (kalman && k != 1) continue;      // (Kalman) x z vx vz are done; y and vy keep the fixed gains
                    const double pred = st.box[FX + k][tid];
                    const double r = r_f[FX + k][d] - pred;
                    st.box[FX + k][tid] = pred + prm.gain_a * r;
                    st.box[FVX + k][tid] = st.box[FVX + k][tid] + prm.gain_b * r;
                }
#pragma unroll
                for (int k = FH; k <= FL; ++k) {
                    const double s = st.box[k][tid];
                    st.box[k][tid] = s + prm.gain_c * (r_f[k][d] - s);
                }
                const double ry = st.box[FRY][tid];
                double delta = wrap(r_f[FRY][d] - ry);
                if (delta >= kPi / 2.0) delta -= kPi;
                if (delta < -(kPi / 2.0)) delta += kPi;
                st.box[FRY][tid] = wrap(ry + prm.gain_a * delta);
                st.hits[tid] += 1;
                st.misses[tid] = 0;
                st.score[tid] = r_score[d];
                r_slot[d] = (int16_t)tid;
            } else {
                const int misses = st.misses[tid] + 1;
                st.misses[tid] = misses;
                if (misses > prm.max_age) {
                    st.id1[tid] = 0; st.hits[tid] = 0; st.misses[tid] = 0; st.score[tid] = 0.0f;
#pragma unroll
                    for (int k = 0; k < GPP_TRACK_FIELDS; ++k) st.box[k][tid] = 0.0;
                    if constexpr (kKf) {
#pragma unroll
                        for (int k = 0; k < kCov; ++k) P[k] = 0.0;
                    }
                }
            }
        }
        __syncthreads();
        // ... and the births
        {
            const bool born = r_flag[tid] == 1 && s_mslot[tid] < 0 && (double)r_score[tid] >= prm.birth_score;
            int n_born, n_free;
            const int b = block_rank(born, tid, s_wave, n_born);
            const bool is_free = st.id1[tid] == 0;
            const int a = block_rank(is_free, tid, s_wave, n_free);
            if (is_free) s_free[a] = (int16_t)tid;
            __syncthreads();
            const int next_id = st.next_id;
            if (born && b < n_free) {
                const int t = s_free[b];
                st.id1[t] = next_id + b + 1;
                st.hits[t] = 1; st.misses[t] = 0; st.score[t] = r_score[tid];
#pragma unroll
                for (int k = 0; k < 7; ++k) st.box[k][t] = r_f[k][tid];
                st.box[FVX][t] = 0.0; st.box[FVY][t] = 0.0; st.box[FVZ][t] = 0.0;
                r_slot[tid] = (int16_t)t;
                if constexpr (kKf) s_mrow[t] = (int16_t)tid;         // (idle behind phase 5: the slot's thread finds its row here)
            }
            __syncthreads();                             // (everyone has read next_id)
            if constexpr (kKf) {
                if (is_free && st.id1[tid] != 0) {       // born into this slot: the covariance lives with the slot's thread
                    const int d = s_mrow[tid];
                    born_cov(P, s_R[0][d], s_R[1][d], s_R[2][d], kfa.p.birth_speed);
                }
            }
            if (tid == 0) {
                st.next_id = next_id + (n_born < n_free ? n_born : n_free);
                st.dropped += n_born > n_free ? n_born - n_free : 0;
                st.frames += 1;
            }
        }
        __syncthreads();

        // ---- 6: the outputs
        if (tid < D) {
            const int t = r_slot[tid];
            track_ids[(size_t)f * D + tid] = t < 0 ? -1 : st.id1[t] - 1;
            track_hits[(size_t)f * D + tid] = t < 0 ? 0 : st.hits[t];
            float* w = dst + (size_t)tid * kRow;
            if (dst != src) {
                const uint32_t* from = (const uint32_t*)(src + (size_t)tid * kRow);
                uint32_t* to = (uint32_t*)w;
                for (int k = 0; k < kRow; ++k) to[k] = from[k];
            }
            if (prm.smooth && t >= 0) {
                const double x = st.box[FX][t], z = st.box[FZ][t], ry = st.box[FRY][t];
                w[19] = (float)x; w[31] = (float)st.box[FY][t]; w[21] = (float)z;
                w[30] = (float)st.box[FH][t]; w[17] = (float)st.box[FW][t]; w[18] = (float)st.box[FL][t];
                w[32] = (float)ry;
                w[25] = (float)wrap(ry - atan2(x, z));
            }
        }
        __syncthreads();
    }

    {
        const uint32_t* from = (const uint32_t*)&st;
        uint32_t* to = (uint32_t*)(states_out + seq);
        for (int k = tid; k < (int)(sizeof(gpp_track_state) / 4); k += kThreads) to[k] = from[k];
    }
    if constexpr (kKf) {
#pragma unroll
        for (int k = 0; k < kCov; ++k) kfa.cov_out[seq].p[k][tid] = P[k];
    }
}

bool unit(double v, bool open_low) { return (open_low ? v > 0.0 : v >= 0.0) && v <= 1.0; }   // (false for NaN)

}  // namespace

extern "C" int gpp_track_state_bytes(size_t* bytes)
{
    if (!bytes) return GPP_ERR_BAD_ARG;
    *bytes = sizeof(gpp_track_state);
    return GPP_OK;
}

extern "C" int gpp_track_workspace_bytes(int S, size_t* bytes)
{
    if (S < 0 || !bytes) return GPP_ERR_BAD_ARG;
    *bytes = plain_bytes(S);
    return GPP_OK;
}

extern "C" int gpp_track_ego_workspace_bytes(int S, int N, size_t* bytes)
{
    if (S < 0 || N < 0 || !bytes) return GPP_ERR_BAD_ARG;
    *bytes = plain_bytes(S) + (size_t)N * kEgoFields * sizeof(double);          // (plain_bytes is a multiple of 8: the records are aligned)
    return GPP_OK;
}

// the entry points: the checks of the contract in their order, then the one launch.  The optimal form asks for the same workspace and
// uses seq_start's copy only.  with_ego: gpp_track_ego_f64 -- the records of the frames inside a sequence are checked here, on the host,
// and copied behind the plain workspace.  kalman: gpp_track_kf_f64 -- not null, and then with_ego says whether records were given; the
// workspace is the ego form's either way
struct kf_host {
    const void* cov_in;
    void* cov_out;
    const gpp_track_kf_params* kf;
};

static int track(bool optimal, bool with_ego, const kf_host* kalman, const double* ego, const float* rows_in, int N, int D,
                 const int32_t* seq_start, int S,
                 const void* state_in, void* state_out, const gpp_track_params* params, float* rows_out, int32_t* track_ids,
                 int32_t* track_hits, void* workspace, size_t workspace_bytes, void* stream)
{
    if (N < 0 || D < 0 || S < 0 || !params || !seq_start) return GPP_ERR_BAD_ARG;
    const gpp_track_params& p = *params;
    if (p.metric != GPP_TRACK_BEV && p.metric != GPP_TRACK_3D && p.metric != GPP_TRACK_DIST && !(kalman && p.metric == GPP_TRACK_MAHA))
        return GPP_ERR_BAD_ARG;
    const bool metres_or_sigmas = p.metric == GPP_TRACK_DIST || p.metric == GPP_TRACK_MAHA;
    if (metres_or_sigmas ? !(p.threshold > 0.0 && __builtin_isfinite(p.threshold)) : !(p.threshold >= 0.0 && p.threshold < 1.0))
        return GPP_ERR_BAD_ARG;
    if (!unit(p.gain_a, true) || !unit(p.gain_b, false) || !unit(p.gain_c, false)) return GPP_ERR_BAD_ARG;
    if (p.max_age < 0 || (p.smooth != 0 && p.smooth != 1) || p.reserved != 0 || __builtin_isnan(p.birth_score)) return GPP_ERR_BAD_ARG;
    if (kalman && (!kalman->kf || gpp_kf::kf_params_bad(*kalman->kf))) return GPP_ERR_BAD_ARG;
    for (int s = 0; s <= S; ++s) {
        const int32_t lo = s == 0 ? 0 : seq_start[s - 1];
        if (seq_start[s] < lo || seq_start[s] > N) return GPP_ERR_BAD_ARG;
    }
    const int f_lo = seq_start[0], f_hi = seq_start[S];              // the frames inside a sequence: seq_start is monotone
    if (with_ego) {
        if (N > 0 && !ego) return GPP_ERR_BAD_ARG;
        for (int f = f_lo; f < f_hi; ++f)
            if (gpp_kf::ego_record_bad(ego + (size_t)f * kEgoFields)) return GPP_ERR_BAD_ARG;
    }
    if (D > kMaxD) return GPP_ERR_UNSUPPORTED;
    if (S > 0 && (!state_in || !state_out)) return GPP_ERR_BAD_ARG;
    if (S > 0 && kalman && (!kalman->cov_in || !kalman->cov_out)) return GPP_ERR_BAD_ARG;
    hipStream_t q = (hipStream_t)stream;
    if (S == 0) return GPP_OK;
    if ((size_t)N * (size_t)D == 0) {
        if (kalman && kalman->cov_out != kalman->cov_in) {
            hipError_t e = hipMemcpyAsync(kalman->cov_out, kalman->cov_in, (size_t)S * sizeof(gpp_track_cov), hipMemcpyDeviceToDevice, q);
            if (e != hipSuccess) return (int)e;
        }
        if (state_out == state_in) return GPP_OK;
        hipError_t e = hipMemcpyAsync(state_out, state_in, (size_t)S * sizeof(gpp_track_state), hipMemcpyDeviceToDevice, q);
        return e == hipSuccess ? GPP_OK : (int)e;
    }
    if (!rows_in || !rows_out || !track_ids || !track_hits || !workspace) return GPP_ERR_BAD_ARG;
    if (((uintptr_t)workspace | (uintptr_t)state_in | (uintptr_t)state_out) & 7u) return GPP_ERR_ALIGN;
    if (kalman && (((uintptr_t)kalman->cov_in | (uintptr_t)kalman->cov_out) & 7u)) return GPP_ERR_ALIGN;
    if (workspace_bytes < plain_bytes(S) + (with_ego || kalman ? (size_t)N * kEgoFields * sizeof(double) : 0)) return GPP_ERR_WORKSPACE;
    hipError_t e = hipMemcpyAsync(workspace, seq_start, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, q);
    if (e != hipSuccess) return (int)e;
    double* ego_copy = (double*)((char*)workspace + plain_bytes(S));                // record f at its own place f: the kernel indexes by frame
    if (with_ego && f_hi > f_lo) {
        e = hipMemcpyAsync(ego_copy + (size_t)f_lo * kEgoFields, ego + (size_t)f_lo * kEgoFields,
                           (size_t)(f_hi - f_lo) * kEgoFields * sizeof(double), hipMemcpyHostToDevice, q);
        if (e != hipSuccess) return (int)e;
    }
    const int32_t* seq = (const int32_t*)workspace;
    const gpp_track_state* in = (const gpp_track_state*)state_in;
    gpp_track_state* out = (gpp_track_state*)state_out;
    double* tables = (double*)((char*)workspace + seq_bytes(S));
    const dim3 grid((unsigned)S), block(kThreads);
    kf_args kfa = {nullptr, nullptr, {}};
    if (kalman) kfa = {(const gpp_track_cov*)kalman->cov_in, (gpp_track_cov*)kalman->cov_out, *kalman->kf};
#define GPP_TRACK_LAUNCH(OPT, EGO, KF) \
    track_kernel<OPT, EGO, KF><<<grid, block, 0, q>>>(rows_in, N, D, seq, in, out, p, rows_out, track_ids, track_hits, OPT ? nullptr : tables, \
                                                      EGO ? ego_copy : nullptr, kfa)
    if (kalman) {
        if (optimal && with_ego) GPP_TRACK_LAUNCH(true, true, true);
        else if (with_ego) GPP_TRACK_LAUNCH(false, true, true);
        else if (optimal) GPP_TRACK_LAUNCH(true, false, true);
        else GPP_TRACK_LAUNCH(false, false, true);
    } else if (optimal && with_ego) GPP_TRACK_LAUNCH(true, true, false);
    else if (with_ego) GPP_TRACK_LAUNCH(false, true, false);
    else if (optimal) GPP_TRACK_LAUNCH(true, false, false);
    else GPP_TRACK_LAUNCH(false, false, false);
#undef GPP_TRACK_LAUNCH
    e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}

extern "C" int gpp_track_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                             const gpp_track_params* params, float* rows_out, int32_t* track_ids, int32_t* track_hits,
                             void* workspace, size_t workspace_bytes, void* stream)
{
    return track(false, false, nullptr, nullptr, rows_in, N, D, seq_start, S, state_in, state_out, params, rows_out, track_ids, track_hits,
                 workspace, workspace_bytes, stream);
}

extern "C" int gpp_track_optimal_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                                     const gpp_track_params* params, float* rows_out, int32_t* track_ids, int32_t* track_hits,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    return track(true, false, nullptr, nullptr, rows_in, N, D, seq_start, S, state_in, state_out, params, rows_out, track_ids, track_hits, workspace,
                 workspace_bytes, stream);
}

extern "C" int gpp_track_ego_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                                 const gpp_track_params* params, const double* ego, int assign, float* rows_out, int32_t* track_ids,
                                 int32_t* track_hits, void* workspace, size_t workspace_bytes, void* stream)
{
    if (assign != GPP_TRACK_ASSIGN_GREEDY && assign != GPP_TRACK_ASSIGN_OPTIMAL) return GPP_ERR_BAD_ARG;
    return track(assign == GPP_TRACK_ASSIGN_OPTIMAL, true, nullptr, ego, rows_in, N, D, seq_start, S, state_in, state_out, params, rows_out,
                 track_ids, track_hits, workspace, workspace_bytes, stream);
}

extern "C" int gpp_track_cov_bytes(size_t* bytes)
{
    if (!bytes) return GPP_ERR_BAD_ARG;
    *bytes = sizeof(gpp_track_cov);
    return GPP_OK;
}

extern "C" int gpp_track_kf_f64(const float* rows_in, int N, int D, const int32_t* seq_start, int S, const void* state_in, void* state_out,
                                const void* cov_in, void* cov_out, const gpp_track_params* params, const gpp_track_kf_params* kf,
                                const double* ego, int assign, float* rows_out, int32_t* track_ids, int32_t* track_hits, void* workspace,
                                size_t workspace_bytes, void* stream)
{
    if (assign != GPP_TRACK_ASSIGN_GREEDY && assign != GPP_TRACK_ASSIGN_OPTIMAL) return GPP_ERR_BAD_ARG;
    const kf_host kalman = {cov_in, cov_out, kf};
    return track(assign == GPP_TRACK_ASSIGN_OPTIMAL, ego != nullptr, &kalman, ego, rows_in, N, D, seq_start, S, state_in, state_out, params,
                 rows_out, track_ids, track_hits, workspace, workspace_bytes, stream);
}
