// infer_ops.hip -- the detector's test-time box logic on the device, batched: what functions/rpn_proposal.py (test config) and
// functions/predict_bbox.py do in numpy between the RPN, the RCNN head and the result, as kernels over B images that never wait for
// the host and never allocate (scda_amd/infer.py records the whole pass into one graph).
//
// Tie rules (numpy's orders, wherever numpy defines one):
//   RPN top-k          score descending, equal scores by ASCENDING anchor index (np.argsort(-s, kind='stable'))
//   per-class sort     score descending, equal scores by DESCENDING row index (a stable ascending sort, reversed: argsort()[::-1])
//   per-image top_n    score descending, equal scores by DESCENDING position in the class-major list of kept rows (same rule)
// Every key below is made unique by putting the tie-break into its low 32 bits, so the selection and the sort have one answer.
//
// Exact arithmetic (compiled with -ffp-contract=off): decode as utils/bbox_helper.py (float64 where numpy promotes, float32 where the
// operands are float32), clip as np.clip, rounded to fp32 where the reference stores into a float32 array.  One exception, stated in
// include/scda_ops.h: the RPN's exp of the float32 size deltas is the correctly rounded float32 exp here, numpy's own SIMD routine there.
#include <math.h>

#include "eval_prims.h"

namespace scda {

// keys that fit one workgroup's LDS (48 KB: pre_nms_top_n = 6000 of the test config); longer lists sort in the caller's workspace
constexpr int kSortCap = 6144;
constexpr int kSortThreads = 1024;

// In-place descending sort of n unique 64-bit keys by all threads of the workgroup (keys in LDS or in global memory: the same
// workgroup reads what it wrote after each barrier).  The bitonic network in its one-direction form (each merge starts with the
// "flip" comparator i <-> i ^ (k - 1), then half-cleaners i <-> i ^ j): every comparator puts the larger key at the lower index, so
// virtual -inf keys at positions >= n never move and the comparators that touch them can be skipped -- no padding storage.
__device__ void sort_desc(unsigned long long *keys, const int n) {
    int npow = 1;
    while (npow < n) npow <<= 1;
    for (int k = 2; k <= npow; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);
            for (int i = threadIdx.x; i < npow; i += blockDim.x) {
                const int l = flip ? (i ^ (k - 1)) : (i ^ j);
                if (l > i && l < n) {
                    const unsigned long long a = keys[i], b = keys[l];
                    if (a < b) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// ---- RPN top-k: one workgroup per image ----------------------------------------------------------------------------------------
// key(k) = fg score bits << 32 | (0xffffffff - k): scores are soft-max outputs (>= 0), so unsigned order of the bits is float order,
// and the larger key is the higher score or, on equal scores, the lower anchor index.  The n-th largest key is found by a radix
// select over its 8 bytes (256-bin histograms in LDS; wave 0 picks the bin), the n keys >= it are compacted (in any order) and sorted.
// prob [B, 2A, fh, fw]: the fg score of anchor k = (h * fw + w) * A + a is channel 2a + 1 at (h, w).
__global__ __launch_bounds__(kSortThreads) void rpn_topk_kernel(const float *__restrict__ prob, const int A, const int plane,
                                                                const int n, unsigned long long *__restrict__ gkeys,
                                                                int *__restrict__ order) {
    __shared__ unsigned long long skeys[kSortCap];
    __shared__ int hist[256];
    __shared__ unsigned long long prefix_s;
    __shared__ int remain_s, count_s;
    const int b = blockIdx.x, tid = threadIdx.x, KA = A * plane;
    const float *pb = prob + (size_t)b * 2 * A * plane;
    auto key_of = [&](const int i) {           // i: position in the channel-major fg planes (coalesced reads)
        const int a = i / plane, cell = i - a * plane;
        const unsigned s = __float_as_uint(pb[(size_t)(2 * a + 1) * plane + cell]);
        return ((unsigned long long)s << 32) | (unsigned long long)(0xffffffffu - (unsigned)(cell * A + a));
    };
    unsigned long long thr = 0;                // n == KA: every key
    if (n < KA) {
        if (tid == 0) { prefix_s = 0; remain_s = n; }
        for (int pass = 7; pass >= 0; --pass) {
            const int shift = 8 * pass;
            const unsigned long long hi_mask = pass == 7 ? 0ull : (~0ull << (shift + 8));
            for (int q = tid; q < 256; q += blockDim.x) hist[q] = 0;
            __syncthreads();
            const unsigned long long prefix = prefix_s;
            for (int i = tid; i < KA; i += blockDim.x) {
                const unsigned long long key = key_of(i);
                if ((key & hi_mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
            }
            __syncthreads();
            if (tid < 64) {                    // wave 0: lane L holds bins 255 - 4L .. 252 - 4L, an inclusive scan from the top bin
                const int lane = tid, want = remain_s;
                int h[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) { h[q] = hist[255 - 4 * lane - q]; s += h[q]; }
                int incl = s;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int v = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += v;
                }
                const unsigned long long hit = __ballot(incl >= want);
                if (lane == __ffsll((long long)hit) - 1) {
                    int c = incl - s;
                    for (int q = 0; q < 4; ++q) {
                        if (c + h[q] >= want) {
                            prefix_s = prefix | ((unsigned long long)(255 - 4 * lane - q) << shift);
                            remain_s = want - c;
                            break;
                        }
                        c += h[q];
                    }
                }
            }
            __syncthreads();
        }
        thr = prefix_s;                        // the n-th largest key itself (keys are unique)
    }
    unsigned long long *keys = n <= kSortCap ? skeys : gkeys + (size_t)b * n;
    if (tid == 0) count_s = 0;
    __syncthreads();
    for (int i = tid; i < KA; i += blockDim.x) {
        const unsigned long long key = key_of(i);
        if (key >= thr) {
            const int pos = atomicAdd(&count_s, 1);
            if (pos < n) keys[pos] = key;      // exactly n keys qualify; the test only guards the buffer
        }
    }
    __syncthreads();
    sort_desc(keys, n);
    for (int j = tid; j < n; j += blockDim.x) order[(size_t)b * n + j] = (int)(0xffffffffu - (unsigned)keys[j]);
}

// ---- RPN decode of the ranked candidates, B images: grid (candidates, images) -----------------------------------------------------
// as box_ops.hip's proposal_decode_kernel, with exp of the float32 size deltas evaluated here: float64 exp rounded once to fp32, the
// correctly rounded float32 exp (numpy's routine is within a few ulp of it; see include/scda_ops.h)
__global__ __launch_bounds__(256) void rpn_decode_kernel(const int *__restrict__ order, const int n, const double *__restrict__ anchors64,
                                                         const float *__restrict__ loc, const float *__restrict__ prob, const int A,
                                                         const int plane, const float *__restrict__ info, const int info_stride,
                                                         const double min_size, float *__restrict__ props5,
                                                         unsigned char *__restrict__ ok) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= n) return;
    const size_t row = (size_t)b * n + j;
    const int k = min(max(order[row], 0), A * plane - 1), a = k % A, cell = k / A;     // (clamp: a guard, order is in range)
    const float *lb = loc + (size_t)b * 4 * A * plane, *pb = prob + (size_t)b * 2 * A * plane;
    const double *r = anchors64 + (size_t)k * 4;
    const double d0 = lb[(size_t)(a * 4 + 0) * plane + cell], d1 = lb[(size_t)(a * 4 + 1) * plane + cell];
    const float ew = (float)exp((double)lb[(size_t)(a * 4 + 2) * plane + cell]);
    const float eh = (float)exp((double)lb[(size_t)(a * 4 + 3) * plane + cell]);
    const double img_h = info[(size_t)b * info_stride], img_w = info[(size_t)b * info_stride + 1];
    const double rcx = (r[0] + r[2]) / 2., rcy = (r[1] + r[3]) / 2., rw = r[2] - r[0], rh = r[3] - r[1];
    const double cx = d0 * rw + rcx, cy = d1 * rh + rcy, w = (double)ew * rw, h = (double)eh * rh;
    double x1 = cx - w / 2., y1 = cy - h / 2., x2 = cx + w / 2., y2 = cy + h / 2.;
    x1 = fmin(fmax(x1, 0.), img_w - 1.); y1 = fmin(fmax(y1, 0.), img_h - 1.);
    x2 = fmin(fmax(x2, 0.), img_w - 1.); y2 = fmin(fmax(y2, 0.), img_h - 1.);
    float *o = props5 + row * 5;
    o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)x2; o[3] = (float)y2;
    o[4] = pb[(size_t)(a * 2 + 1) * plane + cell];
    ok[row] = (x2 - x1 + 1. >= min_size) && (y2 - y1 + 1. >= min_size);
}

// fixed-capacity proposals: rows i < count_b = min(num[b], P) of image b are its kept boxes in NMS order; the rest are the degenerate
// RoI (b, 0, 0, 0, 0) (score 0 in props6), a valid one-pixel RoI for the head, ignored by everything after it
__global__ __launch_bounds__(256) void rpn_gather_kernel(const float *__restrict__ props5, const int n, const long long *__restrict__ keep,
                                                         const long long *__restrict__ num, const int P, float *__restrict__ rois5,
                                                         float *__restrict__ props6, int *__restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= P) return;
    const int cnt = (int)min((long long)P, num[b]);
    if (i == 0) counts[b] = cnt;
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < cnt) {
        const float *src = props5 + ((size_t)b * n + (size_t)keep[(size_t)b * n + i]) * 5;
#pragma unroll
        for (int c = 0; c < 5; ++c) v[c] = src[c];
    }
    const size_t row = (size_t)b * P + i;
    rois5[row * 5] = (float)b;
    props6[row * 6] = (float)b;
#pragma unroll
    for (int c = 0; c < 4; ++c) { rois5[row * 5 + 1 + c] = v[c]; props6[row * 6 + 1 + c] = v[c]; }
    props6[row * 6 + 5] = v[4];
}

// ---- box prediction: functions/predict_bbox.py:13-66 ---------------------------------------------------------------------------
struct BoxNorm { double std[4], mean[4]; };

// one workgroup per (class c >= 1, image b) = list s = b * (C - 1) + c - 1: the image's real rows (i < roi_counts[b]) that pass the
// threshold, sorted (score desc, row desc), decoded and clipped -> boxes5 [s * P + j] = (x1, y1, x2, y2, score); seg[s] = the
// segment-table row scda_nms_segments_hip reads (first row, length, first mask word)
__global__ __launch_bounds__(256) void box_decode_sort_kernel(const float *__restrict__ rois, const int *__restrict__ roi_counts,
                                                              const int P, const float *__restrict__ prob, const float *__restrict__ loc,
                                                              const int C, const float *__restrict__ info, const int info_stride,
                                                              const BoxNorm norm, const float score_thresh,
                                                              unsigned long long *__restrict__ gkeys, float *__restrict__ boxes5,
                                                              long long *__restrict__ seg) {
    __shared__ unsigned long long skeys[kSortCap];
    __shared__ int count_s;
    const int c = blockIdx.x + 1, b = blockIdx.y, s = b * (C - 1) + blockIdx.x, tid = threadIdx.x;
    const int m = min(roi_counts[b], P);
    unsigned long long *keys = P <= kSortCap ? skeys : gkeys + (size_t)s * P;
    if (tid == 0) count_s = 0;
    __syncthreads();
    for (int i = tid; i < m; i += blockDim.x) {
        const float score = prob[((size_t)b * P + i) * C + c];
        if (score_thresh > 0.f && !(score > score_thresh)) continue;
        keys[atomicAdd(&count_s, 1)] = ((unsigned long long)__float_as_uint(score) << 32) | (unsigned)i;
    }
    __syncthreads();
    const int n = count_s;
    sort_desc(keys, n);
    const float hi_x = info[(size_t)b * info_stride + 1] - 1.f, hi_y = info[(size_t)b * info_stride] - 1.f;  // float32, as numpy's w - 1
    for (int j = tid; j < n; j += blockDim.x) {
        const unsigned long long key = keys[j];
        const size_t r = (size_t)b * P + (unsigned)key;
        const float *ro = rois + r * 5;
        // corner_to_center on the float32 RoIs: float32 arithmetic
        const float rcx = (ro[1] + ro[3]) / 2.f, rcy = (ro[2] + ro[4]) / 2.f, rw = ro[3] - ro[1], rh = ro[4] - ro[2];
        const float *d = loc + r * 4 * C + 4 * c;
        // float32 deltas * float64 stds + float64 means: float64 from here on
        const double d0 = (double)d[0] * norm.std[0] + norm.mean[0], d1 = (double)d[1] * norm.std[1] + norm.mean[1];
        const double d2 = (double)d[2] * norm.std[2] + norm.mean[2], d3 = (double)d[3] * norm.std[3] + norm.mean[3];
        const double cx = d0 * (double)rw + (double)rcx, cy = d1 * (double)rh + (double)rcy;
        const double w = exp(d2) * (double)rw, h = exp(d3) * (double)rh;
        const double hw = w / 2., hh = h / 2.;
        double x1 = cx - hw, y1 = cy - hh, x2 = cx + hw, y2 = cy + hh;
        x1 = fmin(fmax(x1, 0.), (double)hi_x); y1 = fmin(fmax(y1, 0.), (double)hi_y);
        x2 = fmin(fmax(x2, 0.), (double)hi_x); y2 = fmin(fmax(y2, 0.), (double)hi_y);
        float *o = boxes5 + ((size_t)s * P + j) * 5;
        o[0] = (float)x1; o[1] = (float)y1; o[2] = (float)x2; o[3] = (float)y2;
        o[4] = __uint_as_float((unsigned)(key >> 32));
    }
    if (tid == 0) {
        long long *e = seg + 3 * (size_t)s;
        e[0] = (long long)s * P; e[1] = n; e[2] = (long long)s * P * ((P + 63) / 64);
    }
}

// one workgroup per image: the kept rows of all its classes, key = score bits << 32 | class << 16 | rank in the class's kept list
// (= its position in the class-major list: larger key on a tie = later row), sorted; the first top_n become
// det [b, i] = (b, x1, y1, x2, y2, score, class), rows beyond the count zero
__global__ __launch_bounds__(kSortThreads) void box_topn_kernel(const float *__restrict__ boxes5, const long long *__restrict__ keep,
                                                                const long long *__restrict__ num, const int P, const int C,
                                                                const int top_n, unsigned long long *__restrict__ gkeys,
                                                                float *__restrict__ det, int *__restrict__ det_counts) {
    __shared__ unsigned long long skeys[kSortCap];
    __shared__ int count_s;
    const int b = blockIdx.x, tid = threadIdx.x, cap = (C - 1) * P;
    unsigned long long *keys = cap <= kSortCap ? skeys : gkeys + (size_t)b * cap;
    if (tid == 0) count_s = 0;
    __syncthreads();
    for (int c = 1; c < C; ++c) {
        const int s = b * (C - 1) + c - 1;
        const int m = (int)num[s];
        for (int j = tid; j < m; j += blockDim.x) {
            const float score = boxes5[((size_t)s * P + (size_t)keep[(size_t)s * P + j]) * 5 + 4];
            keys[atomicAdd(&count_s, 1)] = ((unsigned long long)__float_as_uint(score) << 32) | ((unsigned)c << 16) | (unsigned)j;
        }
    }
    __syncthreads();
    const int n = count_s;
    sort_desc(keys, n);
    const int out = min(n, top_n);
    if (tid == 0) det_counts[b] = out;
    for (int idx = tid; idx < top_n * 7; idx += blockDim.x) {
        const int i = idx / 7, col = idx - i * 7;
        float v = 0.f;
        if (i < out) {
            const unsigned lo = (unsigned)keys[i];
            const int c = (int)(lo >> 16), j = (int)(lo & 0xffff), s = b * (C - 1) + c - 1;
            const float *src = boxes5 + ((size_t)s * P + (size_t)keep[(size_t)s * P + j]) * 5;
            v = col == 0 ? (float)b : col == 6 ? (float)c : src[col - 1];
        }
        det[((size_t)b * top_n + i) * 7 + col] = v;
    }
}

// workspace carving: 256-byte aligned pieces, in the order the entry points use them
struct Carve {
    char *p;
    size_t used = 0;
    explicit Carve(void *base) : p((char *)base) {}
    template <class T> T *take(size_t count) {
        T *r = p ? (T *)(p + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return r;
    }
};

static int topk_n(int KA, int top_n) { return (top_n <= 0 || top_n >= KA) ? KA : top_n; }

// the RPN pieces, in the order scda_rpn_proposals_hip takes them; base == nullptr: sizes only
struct RpnWs {
    unsigned long long *gkeys; int *order; float *props5; unsigned char *ok; long long *keep, *num; void *mask;
    size_t bytes;
    RpnWs(void *base, int B, int KA, int n) {
        Carve w(base);
        gkeys = w.take<unsigned long long>(n > kSortCap ? (size_t)B * n : 1);
        order = w.take<int>((size_t)B * n);
        props5 = w.take<float>((size_t)B * n * 5);
        ok = w.take<unsigned char>((size_t)B * n);
        keep = w.take<long long>((size_t)B * n);
        num = w.take<long long>(B);
        mask = w.take<char>(scda_nms_workspace_bytes(n));
        bytes = w.used;
    }
};

struct BoxWs {
    unsigned long long *gkeys, *gkeys_top; float *boxes5; long long *seg, *keep, *num; void *mask;
    size_t bytes;
    BoxWs(void *base, int B, int P, int C) {
        Carve w(base);
        const size_t S = (size_t)B * (C - 1);
        gkeys = w.take<unsigned long long>(P > kSortCap ? S * P : 1);
        gkeys_top = w.take<unsigned long long>((size_t)(C - 1) * P > (size_t)kSortCap ? S * P : 1);
        boxes5 = w.take<float>(S * P * 5);
        seg = w.take<long long>(S * 3);
        keep = w.take<long long>(S * P);
        num = w.take<long long>(S);
        mask = w.take<uint64_t>(S * P * ((P + 63) / 64));
        bytes = w.used;
    }
};

}  // namespace scda

using namespace scda;

SCDA_API size_t scda_rpn_topk_workspace_bytes(int B, int KA, int top_n) {
    const int n = topk_n(KA, top_n);
    return n > kSortCap ? (size_t)B * n * sizeof(unsigned long long) : 0;
}

SCDA_API int scda_rpn_topk_hip(const float *prob, int B, int A, int fh, int fw, int top_n, int *order, void *ws, void *stream) {
    const long long KA = (long long)A * fh * fw;
    SCDA_CHECK_ARGS(prob && order && B > 0 && A > 0 && fh > 0 && fw > 0 && KA < 0x7fffffffLL, "scda_rpn_topk_hip")
    const int n = topk_n((int)KA, top_n);
    SCDA_CHECK_ARGS(n <= kSortCap || ws, "scda_rpn_topk_hip")
    hipLaunchKernelGGL(rpn_topk_kernel, dim3(B), dim3(kSortThreads), 0, as_stream(stream), prob, A, fh * fw, n,
                       (unsigned long long *)ws, order);
    return launch_status("rpn_topk_kernel");
}

SCDA_API int scda_rpn_decode_batched_hip(const int *order, int n, const double *anchors64, const float *loc, const float *prob, int B,
                                         int A, int fh, int fw, const float *image_info, int info_stride, double min_size,
                                         float *props5, unsigned char *ok, void *stream) {
    SCDA_CHECK_ARGS(order && anchors64 && loc && prob && image_info && props5 && ok && n > 0 && B > 0 && B <= 65535 && A > 0 && fh > 0 &&
                    fw > 0 && info_stride >= 2, "scda_rpn_decode_batched_hip")
    hipLaunchKernelGGL(rpn_decode_kernel, dim3(cdiv(n, 256), B), dim3(256), 0, as_stream(stream), order, n, anchors64, loc, prob, A,
                       fh * fw, image_info, info_stride, min_size, props5, ok);
    return launch_status("rpn_decode_kernel");
}

SCDA_API size_t scda_rpn_proposals_workspace_bytes(int B, int A, int fh, int fw, int top_n) {
    const int KA = A * fh * fw;
    return RpnWs(nullptr, B, KA, topk_n(KA, top_n)).bytes;
}

SCDA_API int scda_rpn_proposals_hip(const float *prob, const float *loc, const double *anchors64, int B, int A, int fh, int fw,
                                    const float *image_info, int info_stride, int pre_nms_top_n, double min_size, float nms_thresh,
                                    int post_nms_top_n, void *ws, float *rois5, float *props6, int *counts, void *stream) {
    SCDA_CHECK_ARGS(prob && loc && anchors64 && image_info && ws && rois5 && props6 && counts && B > 0 && B <= 65535 && A > 0 && fh > 0 &&
                    fw > 0 && (long long)A * fh * fw < 0x7fffffffLL && info_stride >= 2 && post_nms_top_n > 0, "scda_rpn_proposals_hip")
    const int KA = A * fh * fw, n = topk_n(KA, pre_nms_top_n), P = post_nms_top_n;
    RpnWs w(ws, B, KA, n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rpn_topk_kernel, dim3(B), dim3(kSortThreads), 0, st, prob, A, fh * fw, n, w.gkeys, w.order);
    int e = launch_status("rpn_topk_kernel");
    if (e) return e;
    if ((e = scda_rpn_decode_batched_hip(w.order, n, anchors64, loc, prob, B, A, fh, fw, image_info, info_stride, min_size, w.props5,
                                         w.ok, stream)))
        return e;
    for (int b = 0; b < B; ++b)    // one NMS per image (mask + sweep), stopping after P kept boxes; the mask workspace is reused in order
        if ((e = scda_nms_valid_hip(w.props5 + (size_t)b * n * 5, w.ok + (size_t)b * n, n, nms_thresh, w.mask,
                                    (int64_t *)(w.keep + (size_t)b * n), (int64_t *)(w.num + b), P, stream)))
            return e;
    hipLaunchKernelGGL(rpn_gather_kernel, dim3(cdiv(P, 256), B), dim3(256), 0, st, w.props5, n, w.keep, w.num, P, rois5, props6, counts);
    return launch_status("rpn_gather_kernel");
}

SCDA_API size_t scda_box_predict_workspace_bytes(int B, int P, int C) { return BoxWs(nullptr, B, P, C).bytes; }

// the three stages of both entry points; method < 0: hard NMS at nms_thresh, else the soft sweep of soft_nms.hip in its place
static int box_predict(const char *name, const float *rois, const int *roi_counts, int B, int P, const float *prob, const float *loc, int C,
                       const float *image_info, int info_stride, const double *stds_host, const double *means_host, float score_thresh,
                       float nms_thresh, int method, float sigma, float Nt, float threshold, int top_n, void *ws, float *det,
                       int *det_counts, void *stream) {
    if (!(rois && roi_counts && prob && loc && image_info && stds_host && means_host && ws && det && det_counts && B > 0 && P > 0 &&
          P < 65536 && C > 1 && C < 65536 && (long long)B * (C - 1) <= 65535 && info_stride >= 2 && top_n > 0)) {
        set_error("%s: bad arguments", name);
        return SCDA_EINVAL;
    }
    BoxNorm norm;
    for (int q = 0; q < 4; ++q) { norm.std[q] = stds_host[q]; norm.mean[q] = means_host[q]; }
    BoxWs w(ws, B, P, C);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(box_decode_sort_kernel, dim3(C - 1, B), dim3(256), 0, st, rois, roi_counts, P, prob, loc, C, image_info,
                       info_stride, norm, score_thresh, w.gkeys, w.boxes5, w.seg);
    int e = launch_status("box_decode_sort_kernel");
    if (e) return e;
    if (method < 0)
        e = scda_nms_segments_hip(w.boxes5, w.seg, B * (C - 1), P, nms_thresh, w.mask, (int64_t *)w.keep, (int64_t *)w.num, stream);
    else   // rescoring in place: box_topn_kernel reads boxes5[keep[j]] as before, rank j now being the selection order
        e = scda_soft_nms_segments_hip(w.boxes5, w.seg, B * (C - 1), P, method, sigma, Nt, threshold, (int64_t *)w.keep, (int64_t *)w.num,
                                       stream);
    if (e) return e;
    hipLaunchKernelGGL(box_topn_kernel, dim3(B), dim3(kSortThreads), 0, st, w.boxes5, w.keep, w.num, P, C, top_n, w.gkeys_top, det,
                       det_counts);
    return launch_status("box_topn_kernel");
}

SCDA_API int scda_box_predict_hip(const float *rois, const int *roi_counts, int B, int P, const float *prob, const float *loc, int C,
                                  const float *image_info, int info_stride, const double *stds_host, const double *means_host,
                                  float score_thresh, float nms_thresh, int top_n, void *ws, float *det, int *det_counts, void *stream) {
    return box_predict("scda_box_predict_hip", rois, roi_counts, B, P, prob, loc, C, image_info, info_stride, stds_host, means_host,
                       score_thresh, nms_thresh, -1, 0.f, 0.f, 0.f, top_n, ws, det, det_counts, stream);
}

SCDA_API int scda_box_predict_soft_hip(const float *rois, const int *roi_counts, int B, int P, const float *prob, const float *loc, int C,
                                       const float *image_info, int info_stride, const double *stds_host, const double *means_host,
                                       float score_thresh, int top_n, int method, float sigma, float Nt, float threshold, void *ws,
                                       float *det, int *det_counts, void *stream) {
    if (method < 0 || method > 2 || P > scda_soft_nms_capacity()) {      // before anything is launched
        set_error("scda_box_predict_soft_hip: method %d outside 0..2 or P %d above the soft-NMS capacity %d", method, P,
                  scda_soft_nms_capacity());
        return SCDA_EINVAL;
    }
    return box_predict("scda_box_predict_soft_hip", rois, roi_counts, B, P, prob, loc, C, image_info, info_stride, stds_host, means_host,
                       score_thresh, 0.f, method, sigma, Nt, threshold, top_n, ws, det, det_counts, stream);
}
