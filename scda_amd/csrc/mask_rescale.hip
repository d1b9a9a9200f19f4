// mask_rescale.hip -- instance masks at the ORIGINAL image size on the device (gfx950): tools/mask_rcnn_train_val.py:422-423 of the
// reference (write_results_to_file: every pasted float mask resized once more by Pillow to (img_w, img_h), then `> mask_thresh`).
//
// One fused kernel: the pasted plane P of a detection is never written to global memory.  A workgroup owns 32 output columns (one
// word) of one detection and walks down the output rows in blocks of 4; per block it rebuilds in LDS the rows of P its vertical taps
// reach (the paste's two passes, mask_ops.hip), resizes them horizontally and then vertically.  The arithmetic is the paste's: the
// resampler of mask_resample.h, every sample (float) of the left-to-right double sum of (double)pixel * weight, one IEEE operation per
// source operator (-ffp-contract=off).  The rule is stated in include/scda_ops.h and restated in numpy by tests/mask_orig_np.py.
//
// LDS: 4 KB plane + 17.6 KB horizontal pass of the paste + 16 KB P + 3.7 KB Q + 6.6 KB table of the paste's axes + 4.5 KB and 0.6 KB
// tables of the second resize = 53.0 KB.
#include "eval_prims.h"
#include "mask_resample.h"

namespace {
using namespace scda;

constexpr int kMaxIn = 32;                      // largest plane side of the mask head (as mask_ops.hip)
constexpr int kStrip = 32;                      // output columns per workgroup: one word of the packed form
constexpr int kRows = 4;                        // output rows per block
constexpr int kThreads = kResampleThreads;
constexpr int kRatio = 4;                       // largest down-scale n_in / n_out of the second resize the tables below hold
constexpr int kKs2 = 2 * (2 * kRatio) + 1;      // taps per sample of the second resize: ceil(2 * ratio) * 2 + 1 = 17
// input samples that n adjacent output samples reach: < (n - 1) * ratio + 2 * support + 1, support = 2 * ratio
constexpr int kIC = (kStrip - 1) * kRatio + 4 * kRatio + 1;     // 141 columns of P per strip
constexpr int kIR = (kRows - 1) * kRatio + 4 * kRatio + 1;      // 29 rows of P per block
constexpr int kQStride = kStrip + 1;
constexpr int kTaps = 5;                        // table room per sample of the paste's axes: an up-scaled or equal one has 5 taps

enum { FLAG_CAPACITY = 1, FLAG_EMPTY = 2, FLAG_RATIO = 4, FLAG_INPUT = 8 };

// grid (words of an output row, R), 256 threads.  A workgroup writes EVERY row of its 32 columns of detection r's output plane.
template <bool BITS>
__global__ __launch_bounds__(kThreads) void mask_rescale_kernel(const float *__restrict__ rois, int roi_stride, const int *__restrict__ cls,
                                                                const float *__restrict__ planes, int ph, int pw, int H, int W,
                                                                const float *__restrict__ info, int info_stride, int per_image, int Ho,
                                                                int Wo, int Wdo, float threshold, void *__restrict__ out_,
                                                                float *__restrict__ foot, int *__restrict__ status) {
    __shared__ float plane[kMaxIn * kMaxIn];
    __shared__ float tmp1[kMaxIn * kIC];            // the paste's horizontal pass: [ph][the columns of P this strip reaches]
    __shared__ float P[kIR * kIC];                  // the rows of P one block reaches
    __shared__ float Q[kIR * kQStride];             // their second horizontal pass: [rows][strip]
    __shared__ AxisTable<kIC, kTaps>::Lds lds1;
    __shared__ AxisTable<kStrip, kKs2>::Lds ldsh2;
    __shared__ AxisTable<kRows, kKs2>::Lds ldsv2;
    __shared__ int foot_s[4];
    AxisTable<kIC, kTaps> tab1(lds1);               // the paste's taps: horizontal before the row loop, vertical inside it
    AxisTable<kStrip, kKs2> h2(ldsh2);              // the second resize: always tabulated, FLAG_RATIO has emptied what kKs2 cannot hold
    AxisTable<kRows, kKs2> v2(ldsv2);
    static_assert(tab1.holds(kMaxIn), "a down-scaled axis of the largest plane fits the paste's table");
    const int r = blockIdx.y, word = blockIdx.x, oc0 = blockIdx.x * kStrip, t = threadIdx.x;
    const int b = r / per_image;
    // ---- the image (uniform over the workgroup)
    const float *inf = info + (size_t)b * info_stride;
    int h = 0, w = 0, oh = 0, ow = 0, flag = 0;
    bool finite = trunc_ok(inf[0], &h);
    finite = trunc_ok(inf[1], &w) && finite;
    finite = trunc_ok(inf[3], &oh) && finite;
    finite = trunc_ok(inf[4], &ow) && finite;
    if (!finite) {
        flag = FLAG_INPUT;
    } else {
        if (oh > Ho || ow > Wo) flag |= FLAG_CAPACITY;
        if (oh < 1 || ow < 1) flag |= FLAG_EMPTY;
        if (h < 1 || w < 1 || h > H || w > W) flag |= FLAG_INPUT;
        if ((long long)h > (long long)kRatio * oh || (long long)w > (long long)kRatio * ow) flag |= FLAG_RATIO;
    }
    if (word == 0 && t == 0 && r % per_image == 0) status[b] = flag;
    if (flag) oh = ow = 0;                                      // an empty mask: every word below is cleared
    // ---- the RoI and its window [xa, xb) x [ya, yb) inside the h x w image
    const RoiWindow win = read_roi_window(rois, roi_stride, cls, r, !flag);
    int xa = 0, xb = 0, ya = 0, yb = 0;
    bool live = win.live && win.clip_x(0, w, &xa, &xb) && win.clip_y(0, h, &ya, &yb);
    // ---- the footprint: the output samples with a tap inside the window (contiguous on both axes)
    if (t == 0) { foot_s[0] = foot_s[1] = 0x7fffffff; foot_s[2] = foot_s[3] = -1; }
    __syncthreads();
    if (live) {
        // the strip's own columns decide whether it has work; the workgroup of word 0 scans every column, for foot_rois
        const int xlo = word == 0 ? 0 : oc0, xhi = word == 0 ? ow : min(ow, oc0 + kStrip);
        for (int x = xlo + t; x < xhi; x += kThreads) {
            int lo, hi;
            axis_range(w, ow, x, &lo, &hi);
            if (lo < hi && hi > xa && lo < xb) { atomicMin(&foot_s[0], x); atomicMax(&foot_s[2], x); }
        }
        for (int y = t; y < oh; y += kThreads) {
            int lo, hi;
            axis_range(h, oh, y, &lo, &hi);
            if (lo < hi && hi > ya && lo < yb) { atomicMin(&foot_s[1], y); atomicMax(&foot_s[3], y); }
        }
    }
    __syncthreads();
    const int fx1 = foot_s[0], fy1 = foot_s[1], fx2 = foot_s[2], fy2 = foot_s[3];      // (fx: of the columns scanned)
    live = live && fx1 <= fx2 && fy1 <= fy2;
    if (word == 0 && t == 0) {
        float *f = foot + (size_t)r * 5;
        f[0] = (float)b;
        f[1] = live ? (float)fx1 : 0.f; f[2] = live ? (float)fy1 : 0.f;
        f[3] = live ? (float)fx2 : -1.f; f[4] = live ? (float)fy2 : -1.f;
    }
    // ---- what rows outside the footprint hold: O is +0.0f there, its bit is (0.0f > threshold); nothing outside oh x ow
    const int ncol = max(0, min(kStrip, ow - oc0));
    const unsigned int cword = 0.f > threshold ? (ncol >= 32 ? 0xffffffffu : (1u << ncol) - 1u) : 0u;
    auto fill = [&](int ra, int rb) {
        if (BITS) {
            unsigned int *out = (unsigned int *)out_;
            for (int y = ra + t; y < rb; y += kThreads) out[((size_t)r * Ho + y) * Wdo + word] = y < oh ? cword : 0u;
        } else {
            float *out = (float *)out_;
            for (int i = t; i < (rb - ra) * kStrip; i += kThreads) {
                const int y = ra + (i >> 5), c = oc0 + (i & 31);
                if (c < Wo) out[((size_t)r * Ho + y) * Wo + c] = 0.f;
            }
        }
    };
    if (!live || oc0 > fx2 || oc0 + kStrip - 1 < fx1) {
        fill(0, Ho);
        return;
    }
    // ---- the second horizontal pass's taps of this strip and the columns [ic0, ic1) of P they reach; [pa, pb) of them lie in the window
    h2.fill<true>(w, ow, oc0, ncol);
    __syncthreads();
    const int ic0 = h2.first(0), ic1 = h2.first(ncol - 1) + h2.count(ncol - 1), IC = ic1 - ic0;
    const int pa = max(ic0, xa), pb = min(ic1, xb), np = pb - pa;
    // IC > kIC (and IR > kIR below) cannot happen: FLAG_RATIO has emptied every image with n_in > kRatio * n_out, and below that
    // IC < (kStrip - 1) * kRatio + 4 * kRatio + 1 = kIC, IR < kIR -- both tiles are DERIVED from kRatio, kStrip and kRows above, so
    // changing one of those moves them along.  The tests only keep a wrong edit from writing past a tile.
    if (IC > kIC || np <= 0) {
        fill(0, Ho);
        return;
    }
    // ---- the paste's horizontal pass pw -> roi_w for those columns
    for (int i = t; i < ph * pw; i += kThreads) plane[i] = planes[(size_t)r * ph * pw + i];
    tab1.fill<true>(pw, win.w, pa - win.x1, np);
    __syncthreads();
    horizontal_pass(plane, pw, ph, tab1, np, tmp1, kIC, [=](int xi) { return pa - ic0 + xi; });
    // ---- down the rows: blocks before and behind the footprint hold the constant
    const int by0 = fy1 / kRows * kRows, by1 = min((fy2 / kRows + 1) * kRows, Ho);
    fill(0, by0);
    fill(by1, Ho);
    for (int oy0 = by0; oy0 < by1; oy0 += kRows) {
        const int nrow = min(kRows, oh - oy0), rend = min(oy0 + kRows, Ho);
        __syncthreads();                                        // tmp1 is complete / the previous block has been read
        v2.fill<true>(h, oh, oy0, nrow);
        __syncthreads();
        const int ir0 = v2.first(0), ir1 = v2.first(nrow - 1) + v2.count(nrow - 1), IR = ir1 - ir0;
        const int qa = max(ir0, ya), qb = min(ir1, yb), nq = qb - qa;
        if (IR > kIR || nq <= 0) {
            fill(oy0, rend);
            continue;
        }
        // the paste's vertical pass ph -> roi_h for rows [qa, qb) of P; the rest of the tile is the zero plane around the window
        tab1.fill<true>(ph, win.h, qa - win.y1, nq);
        __syncthreads();
        for (int i = t; i < IR * IC; i += kThreads) {
            const int rr = i / IC, cc = i - rr * IC;
            const int row = ir0 + rr, col = ic0 + cc;
            float v = 0.f;
            if (row >= qa && row < qb && col >= pa && col < pb) v = tab1.dot(row - qa, tmp1 + tab1.first(row - qa) * kIC + cc, kIC);
            P[rr * kIC + cc] = v;
        }
        __syncthreads();
        // the second horizontal pass w -> ow of those rows (a row outside the window is zeros: its samples are +0.0f)
        for (int i = t; i < IR * kStrip; i += kThreads) {
            const int rr = i >> 5, ci = i & 31;
            const int row = ir0 + rr;
            float v = 0.f;
            if (ci < ncol && row >= qa && row < qb) v = h2.dot(ci, P + rr * kIC + (h2.first(ci) - ic0), 1);
            Q[rr * kQStride + ci] = v;
        }
        __syncthreads();
        // the second vertical pass h -> oh, the threshold and the store: thread = (row of the block, column of the strip)
        const int j = t >> 5, ci = t & 31;
        const bool valid = j < nrow && ci < ncol;
        const float v = valid ? v2.dot(j, Q + (v2.first(j) - ir0) * kQStride + ci, kQStride) : 0.f;
        if (BITS) {
            const unsigned long long set = __ballot(valid && v > threshold);      // a wave holds two rows of 32 columns
            if (ci == 0 && j < kRows && oy0 + j < rend)
                ((unsigned int *)out_)[((size_t)r * Ho + oy0 + j) * Wdo + word] = (unsigned int)(set >> (32 * (j & 1)));
        } else {
            if (j < kRows && oy0 + j < rend && oc0 + ci < Wo) ((float *)out_)[((size_t)r * Ho + oy0 + j) * Wo + oc0 + ci] = v;
        }
    }
}

}  // namespace

SCDA_API int scda_mask_rescale_max_ratio(void) { return kRatio; }

SCDA_API int scda_mask_rescale_hip(const float *rois, int roi_stride, const int *cls_or_null, const float *planes, int R, int ph, int pw,
                                   int H, int W, const float *image_info, int info_stride, int masks_per_image, int Ho, int Wo,
                                   int packed, float threshold, void *out, float *foot_rois, int *status, void *stream) {
    SCDA_CHECK_ARGS(rois && planes && image_info && out && foot_rois && status && R > 0 && R <= 65535 && roi_stride >= 5 && ph > 0 &&
                    pw > 0 && ph <= kMaxIn && pw <= kMaxIn && H > 0 && W > 0 && info_stride >= 5 && masks_per_image >= 1 && Ho > 0 && Wo > 0,
                    "scda_mask_rescale_hip")
    const int Wdo = (Wo + 31) / 32;
    const dim3 grid(Wdo, R);
    if (packed)
        hipLaunchKernelGGL(mask_rescale_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), rois, roi_stride, cls_or_null, planes, ph,
                           pw, H, W, image_info, info_stride, masks_per_image, Ho, Wo, Wdo, threshold, out, foot_rois, status);
    else
        hipLaunchKernelGGL(mask_rescale_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), rois, roi_stride, cls_or_null, planes, ph,
                           pw, H, W, image_info, info_stride, masks_per_image, Ho, Wo, Wdo, threshold, out, foot_rois, status);
    return launch_status("mask_rescale_kernel");
}
