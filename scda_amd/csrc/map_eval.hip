// map_eval.hip -- Cityscapes mAP on the device (gfx950): the rows validate() writes (tools/faster_rcnn_train_val.py:826-858), utils/cal_mAP.py
// (parse_res, calIoU, cal_mAP) applied to them, and bbox_helper.compute_recall.  The rules R1..R4 are stated in include/scda_ops.h and
// restated in numpy by tests/voc_map_np.py.  Everything is integer work plus single IEEE operations in the reference's order (built
// with -ffp-contract=off and the correctly rounded float32 divide), so ap / max_recall are the reference's bit for bit; the only atomics
// are integer adds (per-class GT counts, the two recall counters) and the sort's LDS histogram counters: two runs give the same bytes.
//
//   map_rows_kernel     per image: the keep_num best live rows (rank under the stable score sort), clip, divide, truncate   (R1)
//   map_match_kernel    per (class, image), one wave: detections in kept order, lanes over the ground truths, first-maximum argmax   (R2)
//   map_recall_kernel   per image: one wave per ground-truth row over the live proposals                                   (R4)
//   map_perm_kernel     the rows in (image, kept order); then radix_sort.h by score (descending) and by class, segment_bounds_kernel
//   map_pr_kernel       per class: cumulative tp, precision envelope, the AP sum left to right by one lane                  (R3)
// The block scan, the envelope step, wave_compact, segment_bounds_kernel and the workspace allocator are those of eval_prims.h.
#include "eval_prims.h"
#include "radix_sort.h"

namespace {
using namespace scda;

constexpr int kMaxPer = 1024, kMaxClasses = 256;

// grid (B), 256 threads
__global__ __launch_bounds__(256) void map_rows_kernel(const float *__restrict__ det, const int *__restrict__ counts, int D,
                                                       const float *__restrict__ info, int info_w, int scale_col, int C, int keep_num,
                                                       int *__restrict__ box, float *__restrict__ score, int *__restrict__ cls,
                                                       int *__restrict__ rank, int *__restrict__ kept, int *__restrict__ tp,
                                                       int *__restrict__ match, int G, int *__restrict__ claimed) {
    __shared__ uint32_t s_key[kMaxPer];         // ascending key = descending float32 score: a total order, so rank is a permutation
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nd = min(max(counts[b], 0), D);
    const float *rows = det + (size_t)b * D * 7;
    for (int d = tid; d < nd; d += 256) s_key[d] = radix::score_descending(rows[d * 7 + 5]);
    __syncthreads();
    const float h = info[(size_t)b * info_w], w = info[(size_t)b * info_w + 1], scale = info[(size_t)b * info_w + scale_col];
    const float xhi = w - 1.0f, yhi = h - 1.0f;
    for (int d = tid; d < D; d += 256) {
        const size_t o = (size_t)b * D + d;
        const bool live = d < nd;
        int r = d;                              // padding rows keep their slot: rank is a permutation of 0..D-1
        int c = 0;
        if (live) {
            const uint32_t s = s_key[d];
            r = 0;
            for (int j = 0; j < nd; ++j) r += (s_key[j] < s || (s_key[j] == s && j < d)) ? 1 : 0;
            c = (int)rows[d * 7 + 6];
        }
        const bool k = live && r < keep_num && c >= 1 && c <= C - 1;
        const float *q = rows + d * 7;
        box[o * 4 + 0] = live ? (int)(fminf(fmaxf(q[1], 0.0f), xhi) / scale) : 0;
        box[o * 4 + 1] = live ? (int)(fminf(fmaxf(q[2], 0.0f), yhi) / scale) : 0;
        box[o * 4 + 2] = live ? (int)(fminf(fmaxf(q[3], 0.0f), xhi) / scale) : 0;
        box[o * 4 + 3] = live ? (int)(fminf(fmaxf(q[4], 0.0f), yhi) / scale) : 0;
        score[o] = live ? q[5] : 0.0f;
        cls[o] = c;
        rank[o] = r;
        kept[o] = k ? 1 : 0;
        tp[o] = 0;
        if (match) match[o] = -1;
    }
    if (claimed)
        for (int g = tid; g < G; g += 256) claimed[(size_t)b * G + g] = 0;
}

struct MatchArgs {
    const int *box, *cls, *rank, *kept;         // [B, D, 4], [B, D] x 3
    const int *gt, *gt_counts;                  // [B, G, 5] (x1, y1, x2, y2, label), [B]
    int D, G;
    double thr;
    int *tp, *gt_num;                           // [B, D], [C]
    int *match, *claimed;                       // [B, D], [B, G] or null
};

// grid (C - 1, B), one wave: image b, class blockIdx.x + 1
__global__ __launch_bounds__(64) void map_match_kernel(MatchArgs p) {
    __shared__ uint16_t s_byrank[kMaxPer], s_dl[kMaxPer], s_gl[kMaxPer];
    __shared__ uint32_t s_claim[kMaxPer / 32];
    const int c = blockIdx.x + 1, b = blockIdx.y, lane = threadIdx.x;
    const int ng = min(max(p.gt_counts[b], 0), p.G);
    const int *gt = p.gt + (size_t)b * p.G * 5;
    const int *cls = p.cls + (size_t)b * p.D, *rank = p.rank + (size_t)b * p.D, *kept = p.kept + (size_t)b * p.D;
    // ---- the class's ground truths in meta order; its kept detections in kept order
    const int Gc = wave_compact(ng, lane, s_gl, 0, [&](int i) { return gt[i * 5 + 4] == c; });
    if (lane == 0 && Gc) atomicAdd(p.gt_num + c, Gc);
    for (int i = lane; i < p.D; i += 64) s_byrank[i] = 0xffffu;
    for (int i = lane; i < kMaxPer / 32; i += 64) s_claim[i] = 0u;
    __syncthreads();
    for (int d = lane; d < p.D; d += 64) {
        const int r = rank[d];
        if (r >= 0 && r < p.D) s_byrank[r] = (uint16_t)d;
    }
    __syncthreads();
    auto mine = [&](int i) { const int d = s_byrank[i]; return d != 0xffff && kept[d] != 0 && cls[d] == c; };
    const int Dc = wave_compact(p.D, lane, s_dl, 0, mine, [&](int i) { return s_byrank[i]; });
    __syncthreads();
    // ---- calIoU and the claim, one detection after the other
    for (int k = 0; k < Dc; ++k) {
        const int d = s_dl[k];
        const int *q = p.box + ((size_t)b * p.D + d) * 4;
        const int x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
        const long long a_dt = (long long)(x2 - x1 + 1) * (long long)(y2 - y1 + 1);
        double best = -1.0;
        int which = 0x7fffffff;
        for (int base = 0; base < Gc; base += 64) {
            const int j = base + lane;
            if (j < Gc) {
                const int *g = gt + s_gl[j] * 5;
                const int ix1 = max(x1, g[0]), iy1 = max(y1, g[1]), ix2 = min(x2, g[2]), iy2 = min(y2, g[3]);
                if (ix1 < ix2 && iy1 < iy2) {
                    const long long inter = (long long)(ix2 - ix1 + 1) * (long long)(iy2 - iy1 + 1);
                    const long long a_gt = (long long)(g[2] - g[0] + 1) * (long long)(g[3] - g[1] + 1);
                    const double v = (double)inter / (double)(a_dt + a_gt - inter);
                    if (v > best) { best = v; which = j; }      // a lane's later rounds replace only on strict >
                }
            }
        }
        // the first maximum across the wave: the larger IoU, on equal IoU the smaller index
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const double ov = __shfl_xor(best, s, 64);
            const int ow = __shfl_xor(which, s, 64);
            if (ov > best || (ov == best && ow < which)) { best = ov; which = ow; }
        }
        const bool found = which != 0x7fffffff;
        const bool free_ = found && !((s_claim[which >> 5] >> (which & 31)) & 1u);
        const bool hit = found && best >= p.thr && free_;
        __syncthreads();
        if (lane == 0) {
            if (hit) s_claim[which >> 5] |= 1u << (which & 31);
            p.tp[(size_t)b * p.D + d] = hit ? 1 : 0;
            if (p.match) p.match[(size_t)b * p.D + d] = hit ? (int)s_gl[which] : -1;
        }
        __syncthreads();
    }
    if (p.claimed)
        for (int j = lane; j < Gc; j += 64) p.claimed[(size_t)b * p.G + s_gl[j]] = (int)((s_claim[j >> 5] >> (j & 31)) & 1u);
}

// bbox_overlaps_kernel's rule (detection_ops.hip): b = the ground truth, q = the proposal
__device__ inline float overlap_f32(const float *b, const float *q) {
    const float box_area = (q[2] - q[0]) * (q[3] - q[1]);
    float o = 0.f;
    const float iw = fminf(b[2], q[2]) - fmaxf(b[0], q[0]);
    if (iw > 0) {
        const float ih = fminf(b[3], q[3]) - fmaxf(b[1], q[1]);
        if (ih > 0) {
            const float ua = (b[2] - b[0]) * (b[3] - b[1]) + box_area - iw * ih;
            o = __fdiv_rn(iw * ih, ua);
        }
    }
    return o;
}

// grid (B), 256 threads = 4 waves, a wave per ground-truth row.  counters: [0] += recalled, [1] += rows given
__global__ __launch_bounds__(256) void map_recall_kernel(const float *__restrict__ props, const int *__restrict__ prop_counts, int P,
                                                         int prop_w, const float *__restrict__ gts, const int *__restrict__ gt_counts,
                                                         int Gr, int gt_w, int *__restrict__ counters) {
    __shared__ int w_cnt[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int np = min(max(prop_counts[b], 0), P), ng = min(max(gt_counts[b], 0), Gr);
    int recalled = 0;
    for (int g = wv; g < ng; g += 4) {
        const float *gb = gts + ((size_t)b * Gr + g) * gt_w;
        float best = 0.0f;                      // np.max over a row of overlaps >= 0
        for (int i = lane; i < np; i += 64) best = fmaxf(best, overlap_f32(gb, props + ((size_t)b * P + i) * prop_w + 1));
        recalled += __ballot(best > 0.5f) != 0ull ? 1 : 0;
    }
    if (lane == 0) w_cnt[wv] = recalled;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int r = w_cnt[0] + w_cnt[1] + w_cnt[2] + w_cnt[3];
        if (r) atomicAdd(counters, r);
        if (ng) atomicAdd(counters + 1, ng);
    }
}

// ------------------------------------------------------------------------------------------------ accumulation
// perm[i * D + rank] = i * D + d: every image's rows in kept order, the images in the order they were added
__global__ __launch_bounds__(256) void map_perm_kernel(const int *__restrict__ rank, int D, uint32_t *__restrict__ perm, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = rank[i];
    if (r >= 0 && r < D) perm[(size_t)(i / D) * D + r] = (uint32_t)i;
}

struct MapKey {
    int kind;                                   // 1: score (descending), 2: class (0 = the row was not kept)
    int shift;
    const float *score;
    const int *cls, *kept;
    __device__ uint32_t digit(uint32_t e) const {
        const uint32_t v = kind == 1 ? radix::score_descending(score[e]) : (kept[e] ? (uint32_t)cls[e] : 0u);
        return (v >> shift) & 255u;
    }
};

// segment_bounds_kernel's key: the class of a sorted row (0 = not kept).  seg [2, kMaxClasses]
struct ClassKey {
    const uint32_t *perm;
    const int *cls, *kept;
    __device__ int operator()(int i) const { const uint32_t e = perm[i]; return kept[e] ? cls[e] : 0; }
};

struct PrArgs {
    const uint32_t *perm;
    const int *tp, *seg, *sum_gt;
    int *tpc;                                   // [n] cumulative true positives of the sorted rows
    double *term;                               // [n] (rec[v] - rec[v - 1]) * env[v]
    double *ap, *max_recall;                    // [C]
    int *rows;                                  // [C]
};

// grid (C), 256 threads: class blockIdx.x (class 0: no rows by construction)
__global__ __launch_bounds__(256) void map_pr_kernel(PrArgs p) {
    __shared__ uint32_t wave_sums[4];
    __shared__ double w_max[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int start = c ? p.seg[c] : 0, end = c ? p.seg[kMaxClasses + c] : 0;
    const int n = end > start ? end - start : 0;
    if (n == 0) {
        if (tid == 0) { p.ap[c] = 0.0; p.max_recall[c] = 0.0; p.rows[c] = 0; }
        return;
    }
    const uint32_t *perm = p.perm + start;
    int *tpc = p.tpc + start;
    double *term = p.term + start;
    const double sg = (double)p.sum_gt[c];
    // ---- cumulative tp, 256 rows a round
    uint32_t carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int v = base + tid;
        const uint32_t f = v < n ? (uint32_t)p.tp[perm[v]] : 0u;
        uint32_t all;
        const uint32_t inc = block_scan256(f, wave_sums, Add(), carry, &all);
        if (v < n) tpc[v] = (int)(carry + inc);
        carry = all;
        __syncthreads();
    }
    __syncthreads();
    // ---- from the last row backwards: env[v] = max(prec[v..]), the row's term of the AP sum.  fp[v] = v + 1 - tp[v]
    double c_max = -1.0;
    for (int base = 0; base < n; base += 256) {
        const int j = base + tid, v = n - 1 - j;
        double pm = -1.0, rec = 0.0, prev = 0.0;
        if (j < n) {
            const double t = (double)tpc[v], f = (double)(v + 1 - tpc[v]);
            pm = t / (t + f);
            rec = t / sg;
            prev = v > 0 ? (double)tpc[v - 1] / sg : 0.0;
        }
        pm = envelope_step(pm, w_max, &c_max);
        if (j < n) term[v] = v == 0 ? rec * pm : (rec - prev) * pm;
    }
    __syncthreads();
    // ---- the sum left to right, np.max(rec) (a NaN stays)
    if (tid == 0) {
        double a = 0.0, m = (double)tpc[0] / sg;
        for (int v = 0; v < n; ++v) {
            a += term[v];
            const double r = (double)tpc[v] / sg;
            if (!(m != m) && (r != r || r > m)) m = r;
        }
        p.ap[c] = a;
        p.max_recall[c] = m;
        p.rows[c] = n;
    }
}

struct AccLayout { size_t perm_a, perm_b, hist, seg, tpc, term, total; };

AccLayout acc_layout(int n_images, int D) {
    AccLayout l;
    const size_t n = (size_t)n_images * D, tiles = (n + radix::kSortTile - 1) / radix::kSortTile;
    Bump ws;
    l.perm_a = ws.take(n * 4); l.perm_b = ws.take(n * 4);
    l.hist = ws.take(tiles * 256 * 4);
    l.seg = ws.take((size_t)2 * kMaxClasses * 4);
    l.tpc = ws.take(n * 4);
    l.term = ws.take(n * 8);
    l.total = ws.total();
    return l;
}

}  // namespace

SCDA_API int scda_map_rows_hip(const float *detections, const int *detection_counts, int B, int D, const float *image_info, int info_w,
                               int scale_column, int num_classes, int keep_num, int *box, float *score, int *cls, int *rank, int *kept,
                               int *tp, int *dbg_match_or_null, int G, int *dbg_claimed_or_null, void *stream) {
    SCDA_CHECK_ARGS(detections && detection_counts && image_info && box && score && cls && rank && kept && tp, "scda_map_rows_hip")
    SCDA_CHECK_ARGS(B > 0 && B <= 65535 && D > 0 && D <= kMaxPer && info_w >= 2 && scale_column >= 0 && scale_column < info_w &&
                    num_classes >= 2 && num_classes <= kMaxClasses && keep_num > 0 && keep_num <= D && G > 0 && G <= kMaxPer,
                    "scda_map_rows_hip (limits: D, G <= 1024, 2 <= num_classes <= 256, 1 <= keep_num <= D)")
    hipLaunchKernelGGL(map_rows_kernel, dim3(B), dim3(256), 0, as_stream(stream), detections, detection_counts, D, image_info, info_w,
                       scale_column, num_classes, keep_num, box, score, cls, rank, kept, tp, dbg_match_or_null, G, dbg_claimed_or_null);
    return launch_status("map_rows_kernel");
}

SCDA_API int scda_map_match_hip(const int *box, const int *cls, const int *rank, const int *kept, int B, int D, const int *gt_boxes,
                                const int *gt_counts, int G, int num_classes, double iou_thr, int *tp, int *gt_num,
                                int *dbg_match_or_null, int *dbg_claimed_or_null, void *stream) {
    SCDA_CHECK_ARGS(box && cls && rank && kept && gt_boxes && gt_counts && tp && gt_num, "scda_map_match_hip")
    SCDA_CHECK_ARGS(B > 0 && B <= 65535 && D > 0 && D <= kMaxPer && G > 0 && G <= kMaxPer && num_classes >= 2 && num_classes <= kMaxClasses,
                    "scda_map_match_hip (limits: D, G <= 1024, 2 <= num_classes <= 256)")
    const MatchArgs args = {box, cls, rank, kept, gt_boxes, gt_counts, D, G, iou_thr, tp, gt_num, dbg_match_or_null, dbg_claimed_or_null};
    hipLaunchKernelGGL(map_match_kernel, dim3(num_classes - 1, B), dim3(64), 0, as_stream(stream), args);
    return launch_status("map_match_kernel");
}

SCDA_API int scda_map_recall_hip(const float *proposals, const int *proposal_counts, int B, int P, int prop_w, const float *gts,
                                 const int *gt_counts, int Gr, int gt_w, int *counters, void *stream) {
    SCDA_CHECK_ARGS(proposals && proposal_counts && gts && gt_counts && counters, "scda_map_recall_hip")
    SCDA_CHECK_ARGS(B > 0 && B <= 65535 && P > 0 && prop_w >= 5 && Gr > 0 && gt_w >= 4 && (long long)B * P * prop_w < 0x7fffffffLL &&
                    (long long)B * Gr * gt_w < 0x7fffffffLL, "scda_map_recall_hip (proposal rows >= 5 wide, ground-truth rows >= 4 wide)")
    hipLaunchKernelGGL(map_recall_kernel, dim3(B), dim3(256), 0, as_stream(stream), proposals, proposal_counts, P, prop_w, gts, gt_counts,
                       Gr, gt_w, counters);
    return launch_status("map_recall_kernel");
}

SCDA_API size_t scda_map_accumulate_workspace_bytes(int n_images, int D) {
    if (n_images <= 0 || D <= 0 || D > kMaxPer || (long long)n_images * D >= 0x7fffffffLL) return 0;
    return acc_layout(n_images, D).total;
}

SCDA_API int scda_map_accumulate_hip(int n_images, int D, const float *score, const int *cls, const int *rank, const int *kept,
                                     const int *tp, const int *sum_gt, int num_classes, void *ws, double *ap, double *max_recall,
                                     int *rows, void *stream) {
    SCDA_CHECK_ARGS(score && cls && rank && kept && tp && sum_gt && ws && ap && max_recall && rows && (uintptr_t)ws % 16 == 0,
                    "scda_map_accumulate_hip")
    SCDA_CHECK_ARGS(n_images > 0 && D > 0 && D <= kMaxPer && (long long)n_images * D < 0x7fffffffLL && num_classes >= 2 &&
                    num_classes <= kMaxClasses, "scda_map_accumulate_hip (limits: D <= 1024, 2 <= num_classes <= 256)")
    const AccLayout l = acc_layout(n_images, D);
    char *w8 = (char *)ws;
    uint32_t *perm_a = (uint32_t *)(w8 + l.perm_a), *perm_b = (uint32_t *)(w8 + l.perm_b), *hist = (uint32_t *)(w8 + l.hist);
    int *seg = (int *)(w8 + l.seg), *tpc = (int *)(w8 + l.tpc);
    double *term = (double *)(w8 + l.term);
    hipStream_t st = as_stream(stream);
    const int n = n_images * D;
    // rows in (image, kept order): stable passes over the score (descending) and the class finish cal_mAP's order -- equal scores of a
    // class keep the order the images were added in, then the row order
    if (hipMemsetAsync(perm_a, 0, (size_t)n * 4, st) != hipSuccess) return launch_status("scda_map_accumulate_hip (memset)");
    hipLaunchKernelGGL(map_perm_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, rank, D, perm_a, n);
    MapKey key = {1, 0, score, cls, kept};
    perm_a = radix::sort_u32(perm_a, perm_b, n, key, hist, st);
    key.kind = 2; key.shift = 0;
    radix::sort_pass(perm_a, perm_b, n, key, hist, st);
    if (hipMemsetAsync(seg, 0, (size_t)2 * kMaxClasses * 4, st) != hipSuccess) return launch_status("scda_map_accumulate_hip (memset)");
    hipLaunchKernelGGL(segment_bounds_kernel<ClassKey>, dim3(cdiv(n, 256)), dim3(256), 0, st, n, ClassKey{perm_b, cls, kept}, kMaxClasses,
                       seg);
    const PrArgs args = {perm_b, tp, seg, sum_gt, tpc, term, ap, max_recall, rows};
    hipLaunchKernelGGL(map_pr_kernel, dim3(num_classes), dim3(256), 0, st, args);
    return launch_status("map accumulate kernels");
}
