// coco_eval.hip -- COCO AP on the device (gfx950): the detection evaluator of datasets/pycocotools/cocoeval.py (COCOeval.evaluate,
// accumulate, summarize for iouType 'bbox' / 'segm' / 'keypoints', and useCats = 0 for the first two) and bbIou of
// datasets/pycocotools/common/maskApi.c.  The rules are stated in include/scda_ops.h and restated in numpy by tests/coco_eval_np.py and
// tests/coco_kps_np.py.  Everything is integer work plus single IEEE double operations in the reference's order (built with
// -ffp-contract=off), so the arrays are the reference's bit for bit -- but for the exp() of the OKS, whose last bit belongs to the
// implementation --; the only atomics are integer adds (the non-ignored GT counts) and integer LDS histogram counters, so two runs give
// the same bytes.
//
//   det_rows_kernel     per detection slot: xywh and area in double from the float32 corners, score, category (0 = padding)
//   box_iou_kernel      per (image, gt, dt) pair: bbIou
//   kp_rows_kernel      per detection slot of a keypoint run: the box and area of its keypoints' extent, score, category
//   oks_kernel          per (image, gt, dt) pair: computeOks' object keypoint similarity; per GT the keypoint ignore flag
//   prop_rows_kernel    per proposal slot: det_rows_kernel's rows from the RPN proposals, category 1
//   regroup_kernel      useCats = 0, per image: the rows in (category, given) order by a stable counting sort, every live category 1;
//                       regroup_iou_kernel: the image's IoU block in that order
//   match_kernel        per (image, category): ranks, the GT orders, evaluateImg's greedy matching, one lane per (area range, threshold)
//   sort_*_kernel       the stable LSD radix sort of radix_sort.h, 8 bits per pass, over the keys of SortKey
//   gather_kernel       the rows in sorted order (score, rank, match bits); segment_bounds_kernel: the category segments
//   pr_kernel           per (category, area range, maxDets): tp / fp scans, precision envelope, the recall thresholds
//   stats_kernel        the 12 numbers of _summarizeDets, the 10 of _summarizeKps
// The block scan, the envelope step, wave_compact, segment_bounds_kernel and the workspace allocator are those of eval_prims.h.
#include "eval_prims.h"
#include "radix_sort.h"

namespace {
using namespace scda;

constexpr int kMaxT = 16, kMaxA = 8, kMaxM = 4, kMaxRec = 128, kMaxPer = 1024;
constexpr int kMatchThreads = 128;              // >= kMaxT * kMaxA lanes, one per (area range, threshold)
constexpr int kIouLds = 2048;                   // doubles of one (image, category)'s IoU block staged in LDS
constexpr int kGtmWords = kMaxPer / 32;

// grid-stride over B * top_n slots
__global__ __launch_bounds__(256) void det_rows_kernel(const float *__restrict__ det, const int *__restrict__ counts, int B, int top_n,
                                                       const uint32_t *__restrict__ mask_area, int K, double *__restrict__ xywh,
                                                       double *__restrict__ area, float *__restrict__ score, int *__restrict__ cat) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * top_n; i += gridDim.x * blockDim.x) {
        const int b = i / top_n, d = i - b * top_n;
        const float *r = det + (size_t)i * 7;
        const double x = (double)r[1], y = (double)r[2];
        const double w = (double)r[3] - x, h = (double)r[4] - y;
        const bool live = d < counts[b];
        const float c = r[6];
        xywh[(size_t)i * 4 + 0] = x; xywh[(size_t)i * 4 + 1] = y; xywh[(size_t)i * 4 + 2] = w; xywh[(size_t)i * 4 + 3] = h;
        area[i] = mask_area ? (double)mask_area[i] : w * h;
        score[i] = live ? r[5] : 0.0f;
        cat[i] = (live && c >= 1.0f && c <= (float)K) ? (int)c : 0;
    }
}

// grid (cdiv(D * G, 256), B): o[b][g * D + d], d < dt_counts[b], g < gt_counts[b] (the rest is not written)
__global__ __launch_bounds__(256) void box_iou_kernel(const double *__restrict__ dt, const int *__restrict__ dt_counts,
                                                      const double *__restrict__ gt, const int *__restrict__ gt_counts,
                                                      const unsigned char *__restrict__ iscrowd, int D, int G, double *__restrict__ iou) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * G) return;
    const int g = i / D, d = i - g * D;
    if (d >= dt_counts[b] || g >= gt_counts[b]) return;
    const double *p = dt + ((size_t)b * D + d) * 4, *q = gt + ((size_t)b * G + g) * 4;
    const double da = p[2] * p[3], ga = q[2] * q[3];
    const double w = fmin(p[2] + p[0], q[2] + q[0]) - fmax(p[0], q[0]);
    const double h = fmin(p[3] + p[1], q[3] + q[1]) - fmax(p[1], q[1]);
    double o = 0.0;
    if (!(w <= 0.0) && !(h <= 0.0)) {
        const double in = w * h;
        const double u = iscrowd[(size_t)b * G + g] ? da : da + ga - in;
        o = in / u;
    }
    iou[(size_t)b * D * G + i] = o;
}

// grid-stride over B * top_n slots.  kp [B, top_n, Kp, 3] float32 (x, y, anything): loadRes' box of a keypoint result (coco.py:350-357),
// the extent of ALL Kp points; slots at or past the image's count are written as zero rows, whatever their keypoints hold
__global__ __launch_bounds__(256) void kp_rows_kernel(const float *__restrict__ det, const int *__restrict__ counts, int B, int top_n,
                                                      const float *__restrict__ kp, int Kp, int K, double *__restrict__ xywh,
                                                      double *__restrict__ area, float *__restrict__ score, int *__restrict__ cat) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * top_n; i += gridDim.x * blockDim.x) {
        const int b = i / top_n, d = i - b * top_n;
        const float *r = det + (size_t)i * 7, *q = kp + (size_t)i * Kp * 3;
        const bool live = d < counts[b];
        double x0 = 0.0, y0 = 0.0, w = 0.0, h = 0.0;
        if (live) {
            double x1 = x0 = (double)q[0], y1 = y0 = (double)q[1];
            for (int j = 1; j < Kp; ++j) {
                const double x = (double)q[3 * j], y = (double)q[3 * j + 1];
                x0 = fmin(x0, x); x1 = fmax(x1, x); y0 = fmin(y0, y); y1 = fmax(y1, y);
            }
            w = x1 - x0; h = y1 - y0;
        }
        const float c = r[6];
        xywh[(size_t)i * 4 + 0] = x0; xywh[(size_t)i * 4 + 1] = y0; xywh[(size_t)i * 4 + 2] = w; xywh[(size_t)i * 4 + 3] = h;
        area[i] = w * h;
        score[i] = live ? r[5] : 0.0f;
        cat[i] = (live && c >= 1.0f && c <= (float)K) ? (int)c : 0;
    }
}

constexpr int kMaxKp = 32;

// grid (cdiv(D, 256), G, B), 256 threads: one GT against 256 detection slots, one thread per pair; the GT's keypoints, box, area and
// the variances are staged once.  o[b][g * D + d], d < dt_counts[b], g < gt_counts[b] (the rest is not written); the first block of a
// GT also writes ignore[b][g] = iscrowd || num_keypoints == 0
__global__ __launch_bounds__(256) void oks_kernel(const float *__restrict__ dt_kp, const int *__restrict__ dt_counts,
                                                  const double *__restrict__ gt_kp, const double *__restrict__ gt_box,
                                                  const double *__restrict__ gt_area, const int *__restrict__ gt_counts,
                                                  const double *__restrict__ vars, const unsigned char *__restrict__ iscrowd,
                                                  const int *__restrict__ gt_num_kp, int D, int G, int Kp, double *__restrict__ oks,
                                                  unsigned char *__restrict__ ignore) {
    __shared__ double s_g[kMaxKp][3], s_var[kMaxKp];
    const int b = blockIdx.z, g = blockIdx.y, tid = threadIdx.x, d = blockIdx.x * 256 + tid;
    if (g >= min(gt_counts[b], G)) return;      // block-uniform
    if (ignore && blockIdx.x == 0 && tid == 0)
        ignore[(size_t)b * G + g] = (iscrowd[(size_t)b * G + g] != 0 || gt_num_kp[(size_t)b * G + g] == 0) ? 1 : 0;
    const int nd = min(dt_counts[b], D);
    if (blockIdx.x * 256 >= nd) return;         // block-uniform
    const double *gk = gt_kp + ((size_t)b * G + g) * Kp * 3;
    for (int i = tid; i < Kp * 3; i += 256) s_g[i / 3][i % 3] = gk[i];
    for (int i = tid; i < Kp; i += 256) s_var[i] = vars[i];
    __syncthreads();
    if (d >= nd) return;
    int k1 = 0;
    for (int i = 0; i < Kp; ++i) k1 += s_g[i][2] > 0.0 ? 1 : 0;
    const double *bb = gt_box + ((size_t)b * G + g) * 4;
    const double den = gt_area[(size_t)b * G + g] + 2.220446049250313e-16;
    const double x0 = bb[0] - bb[2], x1 = bb[0] + bb[2] * 2.0, y0 = bb[1] - bb[3], y1 = bb[1] + bb[3] * 2.0;
    const float *q = dt_kp + ((size_t)b * D + d) * Kp * 3;
    double sum = 0.0;
    for (int i = 0; i < Kp; ++i) {
        if (k1 > 0 && !(s_g[i][2] > 0.0)) continue;
        const double xd = (double)q[3 * i], yd = (double)q[3 * i + 1];
        double dx, dy;
        if (k1 > 0) {
            dx = xd - s_g[i][0];
            dy = yd - s_g[i][1];
        } else {
            dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
            dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        }
        const double e = (dx * dx + dy * dy) / s_var[i] / den / 2.0;
        sum += exp(-e);
    }
    oks[(size_t)b * D * G + (size_t)g * D + d] = sum / (double)(k1 > 0 ? k1 : Kp);
}

// grid-stride over B * P slots.  prop [B, P, 6] = (b, x1, y1, x2, y2, score): the rows det_rows_kernel writes, category 1 for the slots
// below the image's count.  as_xywh: (x2, y2) taken as (w, h), as utils/coco_eval.py:33-36 hands proposals to COCO
__global__ __launch_bounds__(256) void prop_rows_kernel(const float *__restrict__ prop, const int *__restrict__ counts, int B, int P,
                                                        int as_xywh, double *__restrict__ xywh, double *__restrict__ area,
                                                        float *__restrict__ score, int *__restrict__ cat) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * P; i += gridDim.x * blockDim.x) {
        const int b = i / P, d = i - b * P;
        const float *r = prop + (size_t)i * 6;
        const double x = (double)r[1], y = (double)r[2];
        const double w = as_xywh ? (double)r[3] : (double)r[3] - x, h = as_xywh ? (double)r[4] : (double)r[4] - y;
        const bool live = d < counts[b];
        xywh[(size_t)i * 4 + 0] = x; xywh[(size_t)i * 4 + 1] = y; xywh[(size_t)i * 4 + 2] = w; xywh[(size_t)i * 4 + 3] = h;
        area[i] = w * h;
        score[i] = live ? r[5] : 0.0f;
        cat[i] = live ? 1 : 0;
    }
}

// The stable counting sort of useCats = 0 by one block of 256 threads: perm[0 .. live) = the indices i < n with 1 <= key[i] <= kmax (<= 255) in
// (key ascending, index ascending) order, perm[live .. cap) = -1; -> live.  hist, base: 256 ints, keys: 256 ints, part: 4 ints of LDS
__device__ inline int block_sort_by_category(const int *__restrict__ key, int n, int kmax, int cap, int *__restrict__ perm, int *hist, int *base,
                                             int *keys, int *part) {
    const int tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int c = key[i];
        if (c >= 1 && c <= kmax) atomicAdd(hist + c, 1);
    }
    __syncthreads();
    const int v = hist[tid];
    int live;
    base[tid] = block_scan256(v, part, Add(), 0, &live) - v;
    __syncthreads();
    for (int r = 0; r < n; r += 256) {
        const int i = r + tid;
        int c = i < n ? key[i] : 0;
        c = (c >= 1 && c <= kmax) ? c : 0;
        keys[tid] = c;
        __syncthreads();
        if (c) {
            int before = 0;
            for (int j = 0; j < tid; ++j) before += keys[j] == c ? 1 : 0;
            perm[base[c] + before] = i;
        }
        __syncthreads();
        if (c) atomicAdd(base + c, 1);
        __syncthreads();
    }
    for (int i = live + tid; i < cap; i += 256) perm[i] = -1;
    return live;
}

struct RegroupArgs {
    const int *dt_counts, *gt_counts;           // [B]
    const double *in_xywh, *in_area;            // [B, D, 4], [B, D]: the rows in the order given
    const float *in_score;
    const int *in_cat;
    const int *gt_cat;                          // [B, G]
    const double *gt_area;
    const unsigned char *gt_iscrowd;
    int D, G, K;
    double *xywh, *area;                        // the regrouped rows
    float *score;
    int *cat;
    double *out_gt_area;                        // [B, G]
    unsigned char *out_gt_iscrowd;
    int *out_gt_cat;
    int *perm_d, *perm_g;                       // [B, D], [B, G]: the slot / row given that stands at each regrouped place, -1 behind
};

// grid (B), 256 threads: the two permutations of image b and its rows in that order, category 1 for the live ones
__global__ __launch_bounds__(256) void regroup_kernel(RegroupArgs p) {
    __shared__ int s_hist[256], s_base[256], s_keys[256], s_part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nd = min(p.dt_counts[b], p.D), ng = min(p.gt_counts[b], p.G);
    int *pd = p.perm_d + (size_t)b * p.D, *pg = p.perm_g + (size_t)b * p.G;
    block_sort_by_category(p.in_cat + (size_t)b * p.D, nd, p.K, p.D, pd, s_hist, s_base, s_keys, s_part);
    __syncthreads();
    block_sort_by_category(p.gt_cat + (size_t)b * p.G, ng, p.K, p.G, pg, s_hist, s_base, s_keys, s_part);
    __syncthreads();                            // the block's own global writes are visible to it behind the barrier
    for (int j = tid; j < p.D; j += 256) {
        const int s = pd[j];
        const size_t o = (size_t)b * p.D + j, i = (size_t)b * p.D + (s >= 0 ? s : 0);
        for (int q = 0; q < 4; ++q) p.xywh[o * 4 + q] = s >= 0 ? p.in_xywh[i * 4 + q] : 0.0;
        p.area[o] = s >= 0 ? p.in_area[i] : 0.0;
        p.score[o] = s >= 0 ? p.in_score[i] : 0.0f;
        p.cat[o] = s >= 0 ? 1 : 0;
    }
    for (int j = tid; j < p.G; j += 256) {
        const int s = pg[j];
        const size_t o = (size_t)b * p.G + j, i = (size_t)b * p.G + (s >= 0 ? s : 0);
        p.out_gt_area[o] = s >= 0 ? p.gt_area[i] : 0.0;
        p.out_gt_iscrowd[o] = s >= 0 ? p.gt_iscrowd[i] : (unsigned char)0;
        p.out_gt_cat[o] = s >= 0 ? 1 : 0;
    }
}

// grid (cdiv(D * G, 256), B), behind regroup_kernel: out[g * D + d] = in[perm_g[g] * D + perm_d[d]] for the live places (the rest is
// not written)
__global__ __launch_bounds__(256) void regroup_iou_kernel(const double *__restrict__ in, const int *__restrict__ perm_d,
                                                          const int *__restrict__ perm_g, int D, int G, double *__restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * G) return;
    const int g = i / D, d = i - g * D;
    const int sg = perm_g[(size_t)b * G + g], sd = perm_d[(size_t)b * D + d];
    if (sg < 0 || sd < 0) return;
    out[(size_t)b * D * G + i] = in[(size_t)b * D * G + (size_t)sg * D + sd];
}

struct MatchArgs {
    const double *iou;                          // [B, G * D]
    const int *dt_counts, *dt_cat;              // [B], [B, D]
    const float *score;                         // [B, D]
    const double *dt_area;                      // [B, D]
    const int *gt_counts, *gt_cat;              // [B], [B, G]
    const double *gt_area;                      // [B, G]
    const unsigned char *gt_iscrowd;            // [B, G]
    const unsigned char *gt_ignore;             // [B, G] or null: the GT's own ignore flag where it is not its iscrowd (keypoints)
    const double *iou_thrs, *area_rng;          // [T], [A, 2]
    int D, G, K, T, A, max_det;
    int *rank;                                  // [B, D]
    uint32_t *bits;                             // [B, D, A]: matched (bit t) | ignored (bit 16 + t)
    int *npig, *seen;                           // [K, A], [K]
    int *dbg;                                   // [B, D, A, T] or null
};

// grid (K, B), 128 threads: evaluateImg of image b, category k + 1, for every area range and threshold
__global__ __launch_bounds__(kMatchThreads) void match_kernel(MatchArgs p) {
    __shared__ double s_iou[kIouLds];
    __shared__ uint32_t s_gtm[kGtmWords][kMatchThreads];
    __shared__ uint16_t s_go[kMaxA][kMaxPer];   // per area range: the category's GTs, non-ignored first; bit 15 = crowd
    __shared__ float s_score[kMaxPer];
    __shared__ uint16_t s_dl[kMaxPer], s_gl[kMaxPer], s_sorted[kMaxPer];
    __shared__ uint32_t s_tile[kMatchThreads][2];
    __shared__ int s_cnt[2], s_nni[kMaxA];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nd = min(p.dt_counts[b], p.D), ng = min(p.gt_counts[b], p.G);
    const int *dcat = p.dt_cat + (size_t)b * p.D, *gcat = p.gt_cat + (size_t)b * p.G;
    const unsigned char *crowd = p.gt_iscrowd + (size_t)b * p.G;
    const unsigned char *gign = p.gt_ignore ? p.gt_ignore + (size_t)b * p.G : crowd;
    // ---- this category's detections and ground truths, in the order given
    if (wv == 0) {
        const int c = wave_compact(nd, lane, s_dl, 0, [&](int i) { return dcat[i] == k + 1; });
        if (lane == 0) s_cnt[0] = c;
    } else {
        const int c = wave_compact(ng, lane, s_gl, 0, [&](int i) { return gcat[i] == k + 1; });
        if (lane == 0) s_cnt[1] = c;
    }
    __syncthreads();
    const int Dc = s_cnt[0], Gc = s_cnt[1];
    if (Dc == 0 && Gc == 0) return;
    if (tid == 0) p.seen[k] = 1;
    for (int i = tid; i < Dc; i += kMatchThreads) s_score[i] = p.score[(size_t)b * p.D + s_dl[i]];
    __syncthreads();
    // ---- rank = position under the stable sort on -score; the first max_det take part
    for (int i = tid; i < Dc; i += kMatchThreads) {
        const float s = s_score[i];
        int r = 0;
        for (int j = 0; j < Dc; ++j) r += (s_score[j] > s || (s_score[j] == s && j < i)) ? 1 : 0;
        s_sorted[r] = s_dl[i];
        p.rank[(size_t)b * p.D + s_dl[i]] = r;
    }
    // ---- per area range: _ignore = ignore (iscrowd unless given) || area < lo || area > hi; non-ignored first, otherwise as given
    for (int a = wv; a < p.A; a += kMatchThreads / 64) {
        const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
        const double *ga = p.gt_area + (size_t)b * p.G;
        auto ign = [&](int i) { const int g = s_gl[i]; return gign[g] != 0 || ga[g] < lo || ga[g] > hi; };
        const int n0 = wave_compact(Gc, lane, s_go[a], 0, [&](int i) { return !ign(i); });
        wave_compact(Gc, lane, s_go[a], n0, [&](int i) { return ign(i); });
        if (lane == 0) {
            s_nni[a] = n0;
            if (n0) atomicAdd(p.npig + k * p.A + a, n0);
        }
    }
    __syncthreads();
    const int Dm = min(Dc, p.max_det);
    // s_go holds positions in s_gl; add the crowd flag
    for (int i = tid; i < p.A * Gc; i += kMatchThreads) {
        const int a = i / Gc, j = i - a * Gc;
        const uint32_t pos = s_go[a][j];
        s_go[a][j] = (uint16_t)(pos | (crowd[s_gl[pos]] ? 0x8000u : 0u));
    }
    // the IoU block [Gc, Dm] of the category, rows in s_gl's order, columns in rank order, where it fits
    const bool staged = Gc * Dm <= kIouLds;
    const double *iou = p.iou + (size_t)b * p.D * p.G;
    if (staged)
        for (int i = tid; i < Gc * Dm; i += kMatchThreads) {
            const int j = i / Dm, d = i - j * Dm;
            s_iou[i] = iou[(size_t)s_gl[j] * p.D + s_sorted[d]];
        }
    for (int w = 0; w < (Gc + 31) / 32; ++w) s_gtm[w][tid] = 0u;
    __syncthreads();
    const bool active = tid < p.A * p.T;
    const int a = active ? tid / p.T : 0, t = active ? tid - a * p.T : 0;
    const double thr = active ? fmin(p.iou_thrs[t], 1 - 1e-10) : 0.0;
    const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
    const int nni = s_nni[a];
    uint32_t mbits = 0, ibits = 0;
    for (int d = 0; d < Dm; ++d) {
        const int di = s_sorted[d];
        if (active) {
            double best = thr;
            int m = -1;
            for (int gi = 0; gi < Gc; ++gi) {
                const uint32_t e = s_go[a][gi];
                if (((s_gtm[gi >> 5][tid] >> (gi & 31)) & 1u) && !(e & 0x8000u)) continue;
                if (m > -1 && m < nni && gi >= nni) break;
                const int j = e & 0x7fff;
                const double v = staged ? s_iou[j * Dm + d] : iou[(size_t)s_gl[j] * p.D + di];
                if (v < best) continue;
                best = v;
                m = gi;
            }
            bool ig;
            int row = -1;
            if (m >= 0) {
                s_gtm[m >> 5][tid] |= 1u << (m & 31);
                mbits |= 1u << (d & 31);
                ig = m >= nni;
                row = s_gl[s_go[a][m] & 0x7fff];
            } else {
                const double ar = p.dt_area[(size_t)b * p.D + di];
                ig = ar < lo || ar > hi;
            }
            if (ig) ibits |= 1u << (d & 31);
            if (p.dbg) p.dbg[(((size_t)b * p.D + di) * p.A + a) * p.T + t] = row;
        }
        if ((d & 31) == 31 || d == Dm - 1) {
            // 32 detections done: the lanes' bit columns become per-detection threshold masks
            s_tile[tid][0] = mbits; s_tile[tid][1] = ibits;
            mbits = ibits = 0;
            __syncthreads();
            const int d0 = d & ~31, cnt = d - d0 + 1;
            for (int i = tid; i < cnt * p.A; i += kMatchThreads) {
                const int j = i / p.A, aa = i - j * p.A;
                uint32_t mm = 0, ii = 0;
                for (int tt = 0; tt < p.T; ++tt) {
                    mm |= ((s_tile[aa * p.T + tt][0] >> j) & 1u) << tt;
                    ii |= ((s_tile[aa * p.T + tt][1] >> j) & 1u) << tt;
                }
                p.bits[((size_t)b * p.D + s_sorted[d0 + j]) * p.A + aa] = mm | (ii << 16);
            }
            __syncthreads();
        }
    }
    // detections past max_det take no part: no bits, no match
    for (int i = Dm * p.A + tid; i < Dc * p.A; i += kMatchThreads) {
        const int j = i / p.A, aa = i - j * p.A;
        p.bits[((size_t)b * p.D + s_sorted[j]) * p.A + aa] = 0u;
        if (p.dbg)
            for (int tt = 0; tt < p.T; ++tt) p.dbg[(((size_t)b * p.D + s_sorted[j]) * p.A + aa) * p.T + tt] = -1;
    }
}

// ------------------------------------------------------------------------------------------------ the sort keys (radix_sort.h)
struct SortKey {
    int kind;                                   // 0: image id, 1: score (descending), 2: category (0 = the row takes no part)
    int shift;
    const int *ids;
    const float *score;
    const int *cat, *rank;
    int max_det;
    __device__ uint32_t digit(uint32_t e) const {
        uint32_t v;
        if (kind == 0) {
            v = (uint32_t)ids[e] ^ 0x80000000u;
        } else if (kind == 1) {
            v = radix::score_descending(score[e]);
        } else {
            v = (cat[e] > 0 && rank[e] < max_det) ? (uint32_t)cat[e] : 0u;
        }
        return (v >> shift) & 255u;
    }
};

__global__ __launch_bounds__(256) void iota_kernel(uint32_t *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)i;
}

// rows in (image id, slot) order: the sequence the reference concatenates
__global__ __launch_bounds__(256) void rows_kernel(const uint32_t *__restrict__ img_order, int D, uint32_t *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = img_order[i / D] * (uint32_t)D + (uint32_t)(i % D);
}

// the rows in sorted order.  s_bits [A, n]
__global__ __launch_bounds__(256) void gather_kernel(const uint32_t *__restrict__ perm, int n, const float *__restrict__ score,
                                                     const int *__restrict__ cat, const int *__restrict__ rank,
                                                     const uint32_t *__restrict__ bits, int A, int max_det, float *__restrict__ s_score,
                                                     int *__restrict__ s_rank, int *__restrict__ s_cat, uint32_t *__restrict__ s_bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = perm[i];
    const bool part = cat[e] > 0 && rank[e] < max_det;
    s_score[i] = score[e];
    s_rank[i] = rank[e];
    s_cat[i] = part ? cat[e] : 0;
    for (int a = 0; a < A; ++a) s_bits[(size_t)a * n + i] = part ? bits[(size_t)e * A + a] : 0u;
}

// segment_bounds_kernel's key: the category of a sorted row.  seg [2, K + 1]
struct CatKey {
    const int *s_cat;
    __device__ int operator()(int i) const { return s_cat[i]; }
};

__global__ __launch_bounds__(256) void fill_kernel(double *p, size_t n, double v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

struct PrArgs {
    const float *s_score;
    const int *s_rank;
    const uint32_t *s_bits;
    const int *seg, *npig, *seen, *max_dets;
    const double *rec;
    int n, K, T, A, M, R;
    double *precision, *recall, *scores;
};

// pr_kernel's counts, scanned as one value behind one pair of barriers: tp in the low, fp in the high 32 bits of c; in = the rows with
// rank < maxDets.  12 bytes, so that the four wave partials take the LDS the two arrays took
struct __attribute__((packed, aligned(4))) PrCount {
    unsigned long long c;
    uint32_t in;
    __device__ PrCount operator+(const PrCount &o) const { return {c + o.c, in + o.in}; }
};
__device__ inline PrCount lanes_up(PrCount v, int d) { return {__shfl_up(v.c, d, 64), __shfl_up(v.in, d, 64)}; }

// grid (K * A * M), 256 threads.  The rows are visited from the LAST to the first, so the scans in thread order are suffix scans
__global__ __launch_bounds__(256) void pr_kernel(PrArgs p) {
    __shared__ int cs[kMaxRec];
    __shared__ PrCount w_cnt[4];
    __shared__ double w_max[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = blockIdx.x % p.M, a = (blockIdx.x / p.M) % p.A, k = blockIdx.x / (p.M * p.A);
    const int np = p.npig[k * p.A + a];
    if (!p.seen[k] || np == 0) return;          // the arrays hold -1 already
    const int start = p.seg[k + 1], end = p.seg[p.K + 1 + k + 1];
    const int n = end > start ? end - start : 0;
    const int md = p.max_dets[m];
    // cs[r] = the smallest count c with c / npig >= recThrs[r] (np + 1: none); rc >= thr first holds at the c-th true positive
    for (int r = tid; r < p.R; r += 256) {
        int lo = 0, hi = np + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)mid / (double)np >= p.rec[r]) hi = mid; else lo = mid + 1;
        }
        cs[r] = lo;
    }
    const float *score = p.s_score + start;
    const int *rank = p.s_rank + start;
    const uint32_t *bits = p.s_bits + (size_t)a * p.n + start;
    for (int t = 0; t < p.T; ++t) {
        const size_t o_rec = (((size_t)t * p.K + k) * p.A + a) * p.M + m;
        for (int r = tid; r < p.R; r += 256) {
            const size_t o = ((((size_t)t * p.R + r) * p.K + k) * p.A + a) * p.M + m;
            p.precision[o] = 0.0;
            p.scores[o] = 0.0;
        }
        // ---- totals
        unsigned long long tot = 0;             // tp in the low, fp in the high 32 bits
        uint32_t nin = 0;
        for (int i = tid; i < n; i += 256) {
            const uint32_t w = bits[i];
            const bool in = rank[i] < md, mt = (w >> t) & 1u, ig = (w >> (16 + t)) & 1u;
            nin += in ? 1u : 0u;
            if (in && !ig) tot += mt ? 1ull : (1ull << 32);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) { tot += __shfl_xor(tot, s, 64); nin += __shfl_xor(nin, s, 64); }
        __syncthreads();                        // cs is written; the previous round's use of w_* is over
        if (lane == 0) w_cnt[wv] = {tot, nin};
        __syncthreads();
        tot = w_cnt[0].c + w_cnt[1].c + w_cnt[2].c + w_cnt[3].c;
        nin = w_cnt[0].in + w_cnt[1].in + w_cnt[2].in + w_cnt[3].in;
        const uint32_t tp_tot = (uint32_t)tot, fp_tot = (uint32_t)(tot >> 32);
        if (tid == 0) p.recall[o_rec] = nin ? (double)tp_tot / (double)np : 0.0;
        // ---- from the last row backwards
        PrCount c_cnt = {0ull, 0u};
        double c_max = -1.0;
        for (int base = 0; base < n; base += 256) {
            const int j = base + tid, i = n - 1 - j;
            bool in = false, tp = false, fp = false;
            if (j < n) {
                const uint32_t w = bits[i];
                const bool mt = (w >> t) & 1u, ig = (w >> (16 + t)) & 1u;
                in = rank[i] < md;
                tp = in && !ig && mt;
                fp = in && !ig && !mt;
            }
            const PrCount one = {tp ? 1ull : (fp ? (1ull << 32) : 0ull), in ? 1u : 0u};
            PrCount all_c;
            const PrCount s = block_scan256(one, w_cnt, Add(), c_cnt, &all_c) + c_cnt;      // inclusive suffix counts of the row
            const unsigned long long sc = s.c;
            const uint32_t si = s.in;
            // the row's inclusive prefix counts = totals - the suffix behind it
            const uint32_t tpc = tp_tot - ((uint32_t)sc - (tp ? 1u : 0u)), fpc = fp_tot - ((uint32_t)(sc >> 32) - (fp ? 1u : 0u));
            const uint32_t inc = nin - (si - (in ? 1u : 0u));
            const double tpd = (double)tpc, fpd = (double)fpc;
            const double pm = envelope_step(in ? tpd / (fpd + tpd + 2.220446049250313e-16) : -1.0, w_max, &c_max);
            if (in) {
                // searchsorted(rc, thr, 'left'): the c-th true positive for the thresholds whose count is c, the first row for count 0
                for (int pass = 0; pass < 2; ++pass) {
                    if (pass == 0 ? !tp : inc != 1u) continue;
                    const int c = pass == 0 ? (int)tpc : 0;
                    int lo = 0, hi = p.R;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cs[mid] >= c) hi = mid; else lo = mid + 1; }
                    for (int r = lo; r < p.R && cs[r] == c; ++r) {
                        const size_t o = ((((size_t)t * p.R + r) * p.K + k) * p.A + a) * p.M + m;
                        p.precision[o] = pm;
                        p.scores[o] = (double)score[i];
                    }
                }
            }
            c_cnt = all_c;
        }
        __syncthreads();
    }
}

// grid (n_stats), 256 threads.  spec [n, 4] = (ap, t or -1: all or -2: none, a, m): the mean of the entries > -1, or -1
__global__ __launch_bounds__(256) void stats_kernel(const double *__restrict__ precision, const double *__restrict__ recall, int T, int R,
                                                    int K, int A, int M, const int *__restrict__ spec, double *__restrict__ stats) {
    __shared__ double w_sum[4];
    __shared__ uint32_t w_n[4];
    const int *s = spec + blockIdx.x * 4;
    const int ap = s[0], ts = s[1], a = s[2], m = s[3], tid = threadIdx.x;
    const int nt = ts == -1 ? T : (ts >= 0 ? 1 : 0), t0 = ts >= 0 ? ts : 0, nr = ap ? R : 1;
    const long long total = (long long)nt * nr * K;
    double sum = 0.0;
    uint32_t cnt = 0;
    for (long long i = tid; i < total; i += 256) {
        const int k = (int)(i % K), r = (int)((i / K) % nr), t = t0 + (int)(i / ((long long)K * nr));
        const double v = ap ? precision[((((size_t)t * R + r) * K + k) * A + a) * M + m] : recall[(((size_t)t * K + k) * A + a) * M + m];
        if (v > -1.0) { sum += v; ++cnt; }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sum += __shfl_xor(sum, d, 64); cnt += __shfl_xor(cnt, d, 64); }
    if ((tid & 63) == 0) { w_sum[tid >> 6] = sum; w_n[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        sum = ((w_sum[0] + w_sum[1]) + (w_sum[2] + w_sum[3]));
        cnt = w_n[0] + w_n[1] + w_n[2] + w_n[3];
        stats[blockIdx.x] = cnt ? sum / (double)cnt : -1.0;
    }
}

struct AccLayout { size_t perm_a, perm_b, img_a, img_b, hist, seg, s_score, s_rank, s_cat, s_bits, total; };

AccLayout acc_layout(int n_images, int D, int K, int A) {
    AccLayout l;
    const size_t n = (size_t)n_images * D, tiles = (n + radix::kSortTile - 1) / radix::kSortTile;
    Bump ws;
    l.perm_a = ws.take(n * 4); l.perm_b = ws.take(n * 4);
    l.img_a = ws.take((size_t)n_images * 4); l.img_b = ws.take((size_t)n_images * 4);
    l.hist = ws.take(tiles * 256 * 4);
    l.seg = ws.take((size_t)2 * (K + 1) * 4);
    l.s_score = ws.take(n * 4); l.s_rank = ws.take(n * 4); l.s_cat = ws.take(n * 4);
    l.s_bits = ws.take(n * 4 * A);
    l.total = ws.total();
    return l;
}

}  // namespace

SCDA_API int scda_coco_det_rows_hip(const float *detections, const int *detection_counts, int B, int top_n,
                                    const uint32_t *mask_area_or_null, int K, double *dt_xywh, double *dt_area, float *score, int *cat,
                                    void *stream) {
    SCDA_CHECK_ARGS(detections && detection_counts && dt_xywh && dt_area && score && cat && B > 0 && top_n > 0 && K > 0 &&
                    (long long)B * top_n < 0x7fffffffLL, "scda_coco_det_rows_hip")
    hipLaunchKernelGGL(det_rows_kernel, dim3(ew_grid((long long)B * top_n)), dim3(256), 0, as_stream(stream), detections,
                       detection_counts, B, top_n, mask_area_or_null, K, dt_xywh, dt_area, score, cat);
    return launch_status("det_rows_kernel");
}

SCDA_API int scda_coco_box_iou_hip(const double *dt, const int *dt_counts, const double *gt, const int *gt_counts,
                                   const unsigned char *iscrowd, int B, int D, int G, double *iou, void *stream) {
    SCDA_CHECK_ARGS(dt && dt_counts && gt && gt_counts && iscrowd && iou && B > 0 && B <= 65535 && D > 0 && G > 0 && D <= kMaxPer &&
                    G <= kMaxPer, "scda_coco_box_iou_hip")
    hipLaunchKernelGGL(box_iou_kernel, dim3(cdiv((long long)D * G, 256), B), dim3(256), 0, as_stream(stream), dt, dt_counts, gt,
                       gt_counts, iscrowd, D, G, iou);
    return launch_status("box_iou_kernel");
}

namespace {
int launch_match(const char *name, const double *iou, int B, int D, int G, const int *dt_counts, const int *dt_cat, const float *score,
                 const double *dt_area, const int *gt_counts, const int *gt_cat, const double *gt_area, const unsigned char *gt_iscrowd,
                 const unsigned char *gt_ignore, int K, const double *iou_thrs, int T, const double *area_rng, int A, int max_det, int *rank,
                 uint32_t *bits, int *npig, int *seen, int *dbg, void *stream) {
    // the two checks and messages scda_coco_match_hip always had: the pointers, then the limits
    if (!(iou && dt_counts && dt_cat && score && dt_area && gt_counts && gt_cat && gt_area && gt_iscrowd && iou_thrs && area_rng && rank &&
          bits && npig && seen)) {
        set_error("%s: bad arguments", name);
        return SCDA_EINVAL;
    }
    if (!(B > 0 && B <= 65535 && D > 0 && D <= kMaxPer && G > 0 && G <= kMaxPer && K > 0 && K <= 65535 && T > 0 && T <= kMaxT && A > 0 &&
          A <= kMaxA && max_det > 0)) {
        set_error("%s (limits: D, G <= 1024, T <= 16, A <= 8): bad arguments", name);
        return SCDA_EINVAL;
    }
    const MatchArgs args = {iou, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd, gt_ignore, iou_thrs, area_rng,
                            D, G, K, T, A, max_det, rank, bits, npig, seen, dbg};
    hipLaunchKernelGGL(match_kernel, dim3(K, B), dim3(kMatchThreads), 0, as_stream(stream), args);
    return launch_status("match_kernel");
}
}  // namespace

SCDA_API int scda_coco_match_hip(const double *iou, int B, int D, int G, const int *dt_counts, const int *dt_cat, const float *score,
                                 const double *dt_area, const int *gt_counts, const int *gt_cat, const double *gt_area,
                                 const unsigned char *gt_iscrowd, int K, const double *iou_thrs, int T, const double *area_rng, int A,
                                 int max_det, int *rank, uint32_t *bits, int *npig, int *seen, int *dbg_match_or_null, void *stream) {
    return launch_match("scda_coco_match_hip", iou, B, D, G, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd,
                        nullptr, K, iou_thrs, T, area_rng, A, max_det, rank, bits, npig, seen, dbg_match_or_null, stream);
}

SCDA_API int scda_coco_match_ign_hip(const double *iou, int B, int D, int G, const int *dt_counts, const int *dt_cat, const float *score,
                                     const double *dt_area, const int *gt_counts, const int *gt_cat, const double *gt_area,
                                     const unsigned char *gt_iscrowd, const unsigned char *gt_ignore_or_null, int K,
                                     const double *iou_thrs, int T, const double *area_rng, int A, int max_det, int *rank, uint32_t *bits,
                                     int *npig, int *seen, int *dbg_match_or_null, void *stream) {
    return launch_match("scda_coco_match_ign_hip", iou, B, D, G, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd,
                        gt_ignore_or_null, K, iou_thrs, T, area_rng, A, max_det, rank, bits, npig, seen, dbg_match_or_null, stream);
}

SCDA_API int scda_coco_kp_rows_hip(const float *detections, const int *detection_counts, int B, int top_n, const float *keypoints, int Kp,
                                   int K, double *dt_xywh, double *dt_area, float *score, int *cat, void *stream) {
    SCDA_CHECK_ARGS(detections && detection_counts && keypoints && dt_xywh && dt_area && score && cat && B > 0 && top_n > 0 && K > 0 &&
                    Kp > 0 && Kp <= kMaxKp && (long long)B * top_n < 0x7fffffffLL, "scda_coco_kp_rows_hip")
    hipLaunchKernelGGL(kp_rows_kernel, dim3(ew_grid((long long)B * top_n)), dim3(256), 0, as_stream(stream), detections,
                       detection_counts, B, top_n, keypoints, Kp, K, dt_xywh, dt_area, score, cat);
    return launch_status("kp_rows_kernel");
}

SCDA_API int scda_coco_oks_hip(const float *dt_keypoints, const int *dt_counts, const double *gt_keypoints, const double *gt_boxes,
                               const double *gt_areas, const int *gt_counts, const double *vars, int Kp,
                               const unsigned char *gt_iscrowd_or_null, const int *gt_num_keypoints_or_null, int B, int D, int G,
                               double *oks, unsigned char *gt_ignore_or_null, void *stream) {
    SCDA_CHECK_ARGS(dt_keypoints && dt_counts && gt_keypoints && gt_boxes && gt_areas && gt_counts && vars && oks && Kp > 0 &&
                    Kp <= kMaxKp && B > 0 && B <= 65535 && D > 0 && G > 0 && D <= kMaxPer && G <= kMaxPer &&
                    (!gt_ignore_or_null || (gt_iscrowd_or_null && gt_num_keypoints_or_null)), "scda_coco_oks_hip")
    hipLaunchKernelGGL(oks_kernel, dim3(cdiv(D, 256), G, B), dim3(256), 0, as_stream(stream), dt_keypoints, dt_counts, gt_keypoints,
                       gt_boxes, gt_areas, gt_counts, vars, gt_iscrowd_or_null, gt_num_keypoints_or_null, D, G, Kp, oks,
                       gt_ignore_or_null);
    return launch_status("oks_kernel");
}

SCDA_API int scda_coco_prop_rows_hip(const float *proposals, const int *proposal_counts, int B, int P, int xyxy_as_xywh, double *dt_xywh,
                                     double *dt_area, float *score, int *cat, void *stream) {
    SCDA_CHECK_ARGS(proposals && proposal_counts && dt_xywh && dt_area && score && cat && B > 0 && P > 0 &&
                    (long long)B * P < 0x7fffffffLL, "scda_coco_prop_rows_hip")
    hipLaunchKernelGGL(prop_rows_kernel, dim3(ew_grid((long long)B * P)), dim3(256), 0, as_stream(stream), proposals, proposal_counts, B,
                       P, xyxy_as_xywh, dt_xywh, dt_area, score, cat);
    return launch_status("prop_rows_kernel");
}

SCDA_API int scda_coco_regroup_hip(int B, int D, int G, int K, const int *dt_counts, const double *in_xywh, const double *in_area,
                                   const float *in_score, const int *in_cat, const int *gt_counts, const int *gt_cat,
                                   const double *gt_area, const unsigned char *gt_iscrowd, const double *in_iou, double *dt_xywh,
                                   double *dt_area, float *score, int *cat, double *out_gt_area, unsigned char *out_gt_iscrowd,
                                   int *out_gt_cat, double *out_iou, int *perm_dets, int *perm_gts, void *stream) {
    SCDA_CHECK_ARGS(dt_counts && in_xywh && in_area && in_score && in_cat && gt_counts && gt_cat && gt_area && gt_iscrowd && in_iou &&
                    dt_xywh && dt_area && score && cat && out_gt_area && out_gt_iscrowd && out_gt_cat && out_iou && perm_dets && perm_gts &&
                    in_iou != out_iou && in_xywh != dt_xywh && in_area != dt_area && in_score != score && in_cat != cat &&
                    B > 0 && B <= 65535 && D > 0 && D <= kMaxPer && G > 0 && G <= kMaxPer && K > 0 && K <= 255, "scda_coco_regroup_hip")
    const RegroupArgs args = {dt_counts, gt_counts, in_xywh, in_area, in_score, in_cat, gt_cat, gt_area, gt_iscrowd, D, G, K, dt_xywh,
                              dt_area, score, cat, out_gt_area, out_gt_iscrowd, out_gt_cat, perm_dets, perm_gts};
    hipLaunchKernelGGL(regroup_kernel, dim3(B), dim3(256), 0, as_stream(stream), args);
    hipLaunchKernelGGL(regroup_iou_kernel, dim3(cdiv((long long)D * G, 256), B), dim3(256), 0, as_stream(stream), in_iou,
                       (const int *)perm_dets, (const int *)perm_gts, D, G, out_iou);
    return launch_status("regroup kernels");
}

SCDA_API size_t scda_coco_accumulate_workspace_bytes(int n_images, int D, int K, int A) {
    if (n_images <= 0 || D <= 0 || K <= 0 || A <= 0 || A > kMaxA || (long long)n_images * D >= 0x7fffffffLL) return 0;
    return acc_layout(n_images, D, K, A).total;
}

SCDA_API int scda_coco_accumulate_hip(const int *image_ids, int n_images, int D, const int *cat, const int *rank, const float *score,
                                      const uint32_t *bits, const int *npig, const int *seen, int K, int T, int A,
                                      const double *rec_thrs, int R, const int *max_dets, int M, int max_det_last, void *ws,
                                      double *precision, double *recall, double *scores, void *stream) {
    SCDA_CHECK_ARGS(image_ids && cat && rank && score && bits && npig && seen && rec_thrs && max_dets && ws && precision && recall &&
                    scores && (uintptr_t)ws % 16 == 0, "scda_coco_accumulate_hip")
    SCDA_CHECK_ARGS(n_images > 0 && D > 0 && D <= kMaxPer && (long long)n_images * D < 0x7fffffffLL && K > 0 && K <= 255 && T > 0 &&
                    T <= kMaxT && A > 0 && A <= kMaxA && R > 0 && R <= kMaxRec && M > 0 && M <= kMaxM && max_det_last > 0,
                    "scda_coco_accumulate_hip (limits: K <= 255, T <= 16, A <= 8, M <= 4, R <= 128)")
    const AccLayout l = acc_layout(n_images, D, K, A);
    char *w8 = (char *)ws;
    uint32_t *perm_a = (uint32_t *)(w8 + l.perm_a), *perm_b = (uint32_t *)(w8 + l.perm_b);
    uint32_t *img_a = (uint32_t *)(w8 + l.img_a), *img_b = (uint32_t *)(w8 + l.img_b), *hist = (uint32_t *)(w8 + l.hist);
    int *seg = (int *)(w8 + l.seg), *s_rank = (int *)(w8 + l.s_rank), *s_cat = (int *)(w8 + l.s_cat);
    float *s_score = (float *)(w8 + l.s_score);
    uint32_t *s_bits = (uint32_t *)(w8 + l.s_bits);
    hipStream_t st = as_stream(stream);
    const int n = n_images * D;
    // the images by id, then the rows in (image, slot) order: within an (image, category) equal scores keep the order given, which is
    // their rank order, so stable passes over the score (descending) and the category finish the reference's order
    SortKey key = {0, 0, image_ids, score, cat, rank, max_det_last};
    hipLaunchKernelGGL(iota_kernel, dim3(cdiv(n_images, 256)), dim3(256), 0, st, img_a, n_images);
    img_a = radix::sort_u32(img_a, img_b, n_images, key, hist, st);
    hipLaunchKernelGGL(rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, (const uint32_t *)img_a, D, perm_a, n);
    key.kind = 1;
    perm_a = radix::sort_u32(perm_a, perm_b, n, key, hist, st);
    key.kind = 2; key.shift = 0;
    radix::sort_pass(perm_a, perm_b, n, key, hist, st);
    hipLaunchKernelGGL(gather_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, (const uint32_t *)perm_b, n, score, cat, rank, bits, A,
                       max_det_last, s_score, s_rank, s_cat, s_bits);
    if (hipMemsetAsync(seg, 0, (size_t)2 * (K + 1) * 4, st) != hipSuccess) return launch_status("scda_coco_accumulate_hip (memset)");
    hipLaunchKernelGGL(segment_bounds_kernel<CatKey>, dim3(cdiv(n, 256)), dim3(256), 0, st, n, CatKey{s_cat}, K + 1, seg);
    const size_t np_ = (size_t)T * R * K * A * M, nr_ = (size_t)T * K * A * M;
    hipLaunchKernelGGL(fill_kernel, dim3(ew_grid((long long)np_)), dim3(256), 0, st, precision, np_, -1.0);
    hipLaunchKernelGGL(fill_kernel, dim3(ew_grid((long long)np_)), dim3(256), 0, st, scores, np_, -1.0);
    hipLaunchKernelGGL(fill_kernel, dim3(ew_grid((long long)nr_)), dim3(256), 0, st, recall, nr_, -1.0);
    const PrArgs args = {s_score, s_rank, s_bits, seg, npig, seen, max_dets, rec_thrs, n, K, T, A, M, R, precision, recall, scores};
    hipLaunchKernelGGL(pr_kernel, dim3(K * A * M), dim3(256), 0, st, args);
    return launch_status("coco accumulate kernels");
}

SCDA_API int scda_coco_summarize_hip(const double *precision, const double *recall, int T, int R, int K, int A, int M, const int *spec,
                                     int n_stats, double *stats, void *stream) {
    SCDA_CHECK_ARGS(precision && recall && spec && stats && T > 0 && R > 0 && K > 0 && A > 0 && M > 0 && n_stats > 0 && n_stats <= 64,
                    "scda_coco_summarize_hip")
    hipLaunchKernelGGL(stats_kernel, dim3(n_stats), dim3(256), 0, as_stream(stream), precision, recall, T, R, K, A, M, spec, stats);
    return launch_status("stats_kernel");
}
