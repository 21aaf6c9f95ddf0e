// Matching of detections to labels for the evaluation on gfx950 (MI355X): one thread per detection, one workgroup per image.
//
// Restates what utils/eval.py does on the host with the outputs of one image (_image_rows + _match_bin; the reference's
// utils/eval.py:93-118 and :207-226), per detection, so that nothing runs serially:
//   rank      the number of entries of the image with a higher score, or an equal score and a lower index: the position in the stable
//             descending order.  Entries at or below the threshold rank behind every entry above it, so the rank among all entries is
//             the rank among the kept ones.
//   claim     the reference walks the detections of one (image, bin) best score first; each tries ONE annotation, the first arg-max of
//             its IoU row over the annotations of that bin, and wins it when IoU >= threshold and nobody took it before.  Which
//             annotation a detection tries does not depend on the others, so "nobody took it before" = "no detection of a lower rank
//             tries the same annotation with IoU >= threshold": a minimum over ranks per annotation, here an LDS atomic.
// Table and error layout: include/gpp.h, gpp_eval_match_f32.
//
// Arithmetic: box and keypoint pixels are divided by the scale in float32 (what NumPy does for float32_array / python_float), then
// widened; the IoU is utils/anchors.compute_overlap's float64 sequence, every operation separate (this file is compiled with
// -ffp-contract=off: area_a + area_b - iw * ih must not become an FMA).
//
// Per-thread state lives in named registers; the annotations of the image (box and bin) are staged in LDS once and read by every
// thread at the same address (a broadcast).  No array indexed at run time, no scratch.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>

#include "gpp.h"

namespace {

constexpr int kMaxD = GPP_EVAL_MAX_DETECTIONS;       // one thread per detection: the largest workgroup
constexpr int kMaxA = GPP_EVAL_MAX_ANNOTATIONS;      // LDS: 32 + 4 + 4 KB for the annotations, 4 KB for the scores
constexpr int kAnnCols = GPP_EVAL_ANN_COLS;
constexpr int kErrCols = GPP_EVAL_ERR_COLS;

__global__ __launch_bounds__(kMaxD) void eval_match_kernel(const float* __restrict__ boxes, const float* __restrict__ dims,
                                                           const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ orientations, const float* __restrict__ scales,
                                                           const double* __restrict__ annotations, const int32_t* __restrict__ ann_counts,
                                                           int D, int A, int num_classes, float score_thr, int max_detections,
                                                           double iou_thr, int32_t* __restrict__ table, double* __restrict__ errors,
                                                           int32_t* __restrict__ counts)
{
    __shared__ double s_box[kMaxA * 4];
    __shared__ float s_score[kMaxD];
    __shared__ int s_bin[kMaxA];
    __shared__ int s_first[kMaxA];                   // the lowest rank that claims annotation a with IoU >= threshold
    __shared__ int s_selected;

    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    int n_ann = ann_counts[b];
    n_ann = n_ann < 0 ? 0 : (n_ann > A ? A : n_ann);
    const double* __restrict__ ann = annotations + (size_t)b * A * kAnnCols;

    if (tid == 0) s_selected = 0;
    for (int a = tid; a < n_ann; a += nthreads) {
        const double* __restrict__ r = ann + (size_t)a * kAnnCols;
        s_box[4 * a + 0] = r[0]; s_box[4 * a + 1] = r[1]; s_box[4 * a + 2] = r[2]; s_box[4 * a + 3] = r[3];
        // the host compares the float64 columns with the integers label and orientation: a value that is no such integer is in no bin
        const double c = r[15], o = r[16];
        int bin = -1;
        if (c >= 0.0 && c < (double)num_classes && o >= 0.0 && o < 4.0) {
            const int ci = (int)c, oi = (int)o;
            if ((double)ci == c && (double)oi == o) bin = 4 * ci + oi;
        }
        s_bin[a] = bin;
        s_first[a] = INT_MAX;
    }
    const bool live = tid < D;
    const size_t det = (size_t)b * D + (live ? tid : 0);
    const float score = live ? scores[det] : 0.0f;
    if (live) s_score[tid] = score;
    __syncthreads();

    // selection: above the threshold (strict) and among the first max_detections of the stable descending order
    int rank = 0;
    bool selected = false;
    if (live && score > score_thr) {
        for (int j = 0; j < D; ++j) {
            const float other = s_score[j];
            rank += (other > score || (other == score && j < tid)) ? 1 : 0;
        }
        selected = rank < max_detections;
    }

    int bin = -1, claim = -1;
    bool reaches = false;
    const float scale = scales[b];
    if (selected) {
        const int label = labels[det], o = orientations[det];
        if (label >= 0 && label < num_classes && o >= 0 && o < 4) bin = 4 * label + o;
    }
    if (bin >= 0) {
        const float* __restrict__ bx = boxes + det * 12;
        const double x1 = (double)(bx[0] / scale), y1 = (double)(bx[1] / scale), x2 = (double)(bx[2] / scale), y2 = (double)(bx[3] / scale);
        const double area_a = (x2 - x1) * (y2 - y1);
        double best = -1.0;                          // an IoU is >= 0: the first annotation of the bin is claimed even at IoU 0 (argmax of a zero row)
        for (int a = 0; a < n_ann; ++a) {
            if (s_bin[a] != bin) continue;
            const double ax1 = s_box[4 * a + 0], ay1 = s_box[4 * a + 1], ax2 = s_box[4 * a + 2], ay2 = s_box[4 * a + 3];
            // utils/anchors.compute_overlap, operation for operation
            double iw = fmin(x2, ax2) - fmax(x1, ax1);
            double ih = fmin(y2, ay2) - fmax(y1, ay1);
            iw = iw < 0.0 ? 0.0 : iw;
            ih = ih < 0.0 ? 0.0 : ih;
            const double inter = iw * ih;
            const double area_b = (ax2 - ax1) * (ay2 - ay1);
            double uni = area_a + area_b - inter;
            uni = uni > DBL_EPSILON ? uni : DBL_EPSILON;
            const double iou = inter / uni;
            if (iou > best) { best = iou; claim = a; }          // strict: the FIRST maximum
        }
        reaches = claim >= 0 && best >= iou_thr;
        if (reaches) atomicMin(&s_first[claim], rank);
    }
    if (selected) atomicAdd(&s_selected, 1);
    __syncthreads();

    if (tid == 0) counts[b] = s_selected;
    if (!live) return;
    const bool hit = reaches && s_first[claim] == rank;          // ranks are distinct inside an image
    int32_t* __restrict__ t = table + det * 3;
    t[0] = selected ? bin : -1;
    t[1] = selected ? (hit ? 1 : 0) : -1;
    t[2] = selected ? claim : -1;
    double* __restrict__ e = errors + det * kErrCols;
    if (hit) {
        const float* __restrict__ bx = boxes + det * 12;
        const float* __restrict__ dm = dims + det * 3;
        const double* __restrict__ r = ann + (size_t)claim * kAnnCols;
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = fabs((double)(bx[4 + k] / scale) - r[4 + k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) e[8 + k] = fabs((double)dm[k] - r[12 + k]);
    } else {
#pragma unroll
        for (int k = 0; k < kErrCols; ++k) e[k] = 0.0;
    }
}

}  // namespace

extern "C" int gpp_eval_match_f32(const float* boxes, const float* dims, const float* scores, const int32_t* labels,
                                  const int32_t* orientations, const float* scales, const double* annotations,
                                  const int32_t* ann_counts, int B, int D, int A, int num_classes, float score_thr,
                                  int max_detections, double iou_thr, int32_t* table, double* errors, int32_t* counts, void* stream)
{
    if (B < 0 || D < 0 || A < 0 || num_classes < 0 || max_detections < 0) return GPP_ERR_BAD_ARG;
    if (B == 0 || D == 0) return GPP_OK;
    if (!boxes || !dims || !scores || !labels || !orientations || !scales || !ann_counts || !table || !errors || !counts ||
        (A > 0 && !annotations))
        return GPP_ERR_BAD_ARG;
    if (D > kMaxD || A > kMaxA) return GPP_ERR_UNSUPPORTED;
    const unsigned threads = (unsigned)((D + 63) / 64 * 64);
    eval_match_kernel<<<dim3((unsigned)B), dim3(threads), 0, (hipStream_t)stream>>>(boxes, dims, scores, labels, orientations, scales,
                                                                                    annotations, ann_counts, D, A, num_classes, score_thr,
                                                                                    max_detections, iou_thr, table, errors, counts);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? GPP_OK : (int)e;
}
