// keypoint_ops.hip -- the keypoint branch at test time on the device (gfx950): R x Kp heat maps -> (x, y, score) rows.
//
// The rule (include/scda_ops.h states it; the choice is OURS -- the reference's own heat-map decoder is in its missing
// models/mask_rcnn/mask_rcnn.py): functions/mask.py:21-49 (`predict_masks`: the plane resized to the RoI by Pillow >= 7, a float BICUBIC
// resize, pasted at the RoI's place) followed by numpy's argmax over the part of the window that lies inside the image.  The resize is
// mask_ops.hip's, operation for operation (mask_resample.h, -ffp-contract=off), so every resized value is Pillow's bit for bit; what is
// new is that the values are never written: each thread keeps a running (value, position) pair, a wave and block reduction leaves one
// partial per (column strip, keypoint, RoI) in the workspace and a second small kernel picks the winner among the strips.
//
// Every comparison is `better()`: greater; or equal with a lower row-major position; or NaN against a non-NaN (np.argmax: a NaN is a
// maximum and the first NaN wins).  That is a total order on (value, position) pairs with distinct positions, so the result does not
// depend on the order in which lanes, waves or strips are combined.
//
// LDS.  Planes go up to 64 x 64.  Tabulating a down-scaled axis as mask_ops.hip does (n_in - 1 samples of n_in taps) would take
// 63 * 64 doubles = 32 KB per axis, 113 KB with the plane and the horizontal pass: one workgroup per CU.  Here an up-scaled (or equal)
// axis -- at most 5 taps per sample -- is tabulated, and a down-scaled axis (fewer than 64 output samples, a small window) keeps per
// sample only the first tap, the tap count and the weights' sum, and recomputes bicubic(.) / sum per tap: the same IEEE operations in
// the same order as axis_taps.  16 KB plane + 32 KB horizontal pass + 7.5 KB tables + 3 KB per-sample entries = 58.6 KB.
#include "eval_prims.h"
#include "mask_resample.h"      // bicubic, axis_ksize, axis_taps, trunc_ok

#include <climits>

namespace {
using namespace scda;

constexpr int kMaxIn = 64;                      // largest plane side (the keypoint head gives 56)
constexpr int kStrip = 128;                     // image columns per workgroup
constexpr int kRows = 64;                       // window rows per vertical-table refill
constexpr int kThreads = 256;
constexpr int kUpTaps = 5;                      // taps of a sample of an up-scaled or equal axis: ceil(2.0) * 2 + 1

struct Best { float v; int at; };               // a resized value and its position y * W + x in the image; INT_MAX: none yet

// np.argmax's order on (value, row-major position): a wins against b
__device__ inline bool better(float av, int aat, float bv, int bat) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (an || av == bv) return aat < bat;
    return av > bv;
}

// one sample of a DOWN-scaled axis n_in -> n_out (n_out < n_in): first tap, tap count and the left-to-right sum of the raw weights,
// as axis_taps computes them
__device__ inline void axis_sum(int n_in, int n_out, int xx, int ks, int *first, int *count, double *sum) {
    const double scale = (double)n_in / n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    int n = xmax - xmin;
    if (n > ks) n = ks;
    if (n < 0) n = 0;
    double ww = 0.0;
    for (int k = 0; k < n; ++k) ww += bicubic((k + xmin - center + 0.5) * ss);
    *first = xmin; *count = n; *sum = ww;
}

// tap k of that sample: axis_taps' w[k] after its normalisation
__device__ inline double axis_weight(int n_in, int n_out, int xx, int first, int k, double sum) {
    const double scale = (double)n_in / n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    double w = bicubic((k + first - center + 0.5) * ss);
    if (sum != 0.0) w /= sum;
    return w;
}

__device__ inline Best wave_best(Best b) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(b.v, d, 64);
        const int oat = __shfl_xor(b.at, d, 64);
        if (better(ov, oat, b.v, b.at)) { b.v = ov; b.at = oat; }
    }
    return b;
}

// grid (column strips, Kp, R), 256 threads.  A workgroup owns columns [c0, c0 + 128) of the window of RoI r and heat map k and leaves
// the best (value, position) of the visible part of them in part[(r * Kp + k) * strips + strip] ({-inf, INT_MAX}: nothing visible).
__global__ __launch_bounds__(kThreads) void keypoint_strip_kernel(const float *__restrict__ rois, int roi_stride, const int *__restrict__ cls,
                                                                  const float *__restrict__ heat, long long sr, long long sk, long long sh,
                                                                  long long sw, int Kp, int ph, int pw, int H, int W,
                                                                  Best *__restrict__ part) {
    __shared__ float plane[kMaxIn * kMaxIn];
    __shared__ float tmp[kMaxIn * kStrip];                         // the horizontal pass: [ph][this strip's columns]
    __shared__ double hw[kStrip * kUpTaps], vw[kRows * kUpTaps];   // the weights of an up-scaled or equal axis
    __shared__ double hsum[kMaxIn], vsum[kMaxIn];                  // the weights' sums of a down-scaled axis (fewer than kMaxIn samples)
    __shared__ int hfirst[kStrip], hcount[kStrip], vfirst[kRows], vcount[kRows];
    __shared__ Best wave_part[kThreads / 64];
    const int r = blockIdx.z, k = blockIdx.y, c0 = blockIdx.x * kStrip, t = threadIdx.x;
    // ---- the RoI (uniform over the workgroup), as mask_paste_kernel reads it
    const float *roi = rois + (size_t)r * roi_stride;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    bool live = !(cls && cls[r] < 0);
    live = trunc_ok(roi[1], &x1) && live;
    live = trunc_ok(roi[2], &y1) && live;
    live = trunc_ok(roi[3], &x2) && live;
    live = trunc_ok(roi[4], &y2) && live;
    int roi_w = 0, roi_h = 0;
    if (live) {
        roi_w = x2 - x1 + 1; roi_h = y2 - y1 + 1;
        live = roi_w > 0 && roi_h > 0;
    }
    // columns [ca, cb) of this strip and rows [ya, yb) of the image lie inside the window
    int ca = 0, cb = 0, ya = 0, yb = 0;
    if (live) {
        ca = x1 > c0 ? x1 : c0;
        cb = min(min(x1 + roi_w, W), c0 + kStrip);
        ya = y1 > 0 ? y1 : 0;
        yb = min(y1 + roi_h, H);
        live = ca < cb && ya < yb;
    }
    Best best = {-INFINITY, INT_MAX};
    if (live) {
        const int na = cb - ca;                                    // 1 .. kStrip
        const bool down_h = roi_w < pw, down_v = roi_h < ph;       // a down-scaled axis has fewer than kMaxIn samples in all
        const int ksh = axis_ksize(pw, roi_w), ksv = axis_ksize(ph, roi_h);     // <= kUpTaps unless down-scaled
        const float *src_plane = heat + r * sr + k * sk;
        for (int i = t; i < ph * pw; i += kThreads) {
            const int y = i / pw, x = i - y * pw;
            plane[i] = src_plane[y * sh + x * sw];
        }
        for (int i = t; i < na; i += kThreads) {
            if (down_h) axis_sum(pw, roi_w, ca + i - x1, ksh, &hfirst[i], &hcount[i], &hsum[i]);
            else axis_taps(pw, roi_w, ca + i - x1, ksh, &hfirst[i], &hcount[i], &hw[i * kUpTaps]);
        }
        __syncthreads();
        for (int i = t; i < ph * na; i += kThreads) {
            const int row = i / na, xa = i - row * na;
            const int first = hfirst[xa], n = hcount[xa];
            const float *src = plane + row * pw + first;
            double s = 0.0;
            if (down_h) {
                const double sum = hsum[xa];
                for (int q = 0; q < n; ++q) s += (double)src[q] * axis_weight(pw, roi_w, ca + xa - x1, first, q, sum);
            } else {
                const double *w = hw + xa * kUpTaps;
                for (int q = 0; q < n; ++q) s += (double)src[q] * w[q];
            }
            tmp[row * kStrip + xa] = (float)s;
        }
        // ---- the vertical pass over the visible rows, kRows at a time; nothing is stored but each thread's best
        for (int ybase = ya; ybase < yb; ybase += kRows) {
            const int nv = min(yb - ybase, kRows);
            __syncthreads();                                       // tmp is complete / the previous refill has been read
            for (int i = t; i < nv; i += kThreads) {
                if (down_v) axis_sum(ph, roi_h, ybase + i - y1, ksv, &vfirst[i], &vcount[i], &vsum[i]);
                else axis_taps(ph, roi_h, ybase + i - y1, ksv, &vfirst[i], &vcount[i], &vw[i * kUpTaps]);
            }
            __syncthreads();
            for (int i = t; i < nv * na; i += kThreads) {          // row-major over this refill's part of the strip
                const int ty = i / na, xa = i - ty * na;
                const int first = vfirst[ty], n = vcount[ty];
                const float *col = tmp + first * kStrip + xa;
                double s = 0.0;
                if (down_v) {
                    const double sum = vsum[ty];
                    for (int q = 0; q < n; ++q) s += (double)col[q * kStrip] * axis_weight(ph, roi_h, ybase + ty - y1, first, q, sum);
                } else {
                    const double *w = vw + ty * kUpTaps;
                    for (int q = 0; q < n; ++q) s += (double)col[q * kStrip] * w[q];
                }
                const float v = (float)s;
                const int at = (ybase + ty) * W + ca + xa;
                if (better(v, at, best.v, best.at)) { best.v = v; best.at = at; }
            }
        }
    }
    best = wave_best(best);
    if ((t & 63) == 0) wave_part[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < kThreads / 64; ++q)
            if (better(wave_part[q].v, wave_part[q].at, best.v, best.at)) best = wave_part[q];
        part[((size_t)r * Kp + k) * gridDim.x + blockIdx.x] = best;
    }
}

// one thread per (RoI, keypoint): the winner among the strips -> (x, y, value), or (0, 0, 0) when nothing of the window is visible
__global__ void keypoint_pick_kernel(const Best *__restrict__ part, int n, int strips, int W, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Best best = {-INFINITY, INT_MAX};
    for (int s = 0; s < strips; ++s) {
        const Best b = part[(size_t)i * strips + s];
        if (better(b.v, b.at, best.v, best.at)) best = b;
    }
    float *o = out + (size_t)i * 3;
    if (best.at == INT_MAX) {
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    } else {
        const int y = best.at / W;
        o[0] = (float)(best.at - y * W); o[1] = (float)y; o[2] = best.v;
    }
}

}  // namespace

SCDA_API size_t scda_keypoint_decode_workspace_bytes(int R, int Kp, int W) {
    if (R <= 0 || Kp <= 0 || W <= 0) return 0;
    return align256((size_t)R * Kp * cdiv(W, kStrip) * sizeof(Best));
}

SCDA_API int scda_keypoint_decode_hip(const float *rois, int roi_stride, const int *cls_or_null, const float *heat, long long stride_r,
                                      long long stride_k, long long stride_h, long long stride_w, int R, int Kp, int ph, int pw, int H,
                                      int W, void *workspace, float *out, void *stream) {
    SCDA_CHECK_ARGS(rois && heat && workspace && out && R > 0 && R <= 65535 && Kp > 0 && Kp <= 65535 && roi_stride >= 5 && ph > 0 &&
                    pw > 0 && ph <= kMaxIn && pw <= kMaxIn && H > 0 && W > 0 && (long long)H * W < 0x7fffffffLL &&
                    (long long)R * Kp < 0x7fffffffLL && stride_r >= 0 && stride_k >= 0 && stride_h >= 0 && stride_w >= 0,
                    "scda_keypoint_decode_hip")
    const int strips = cdiv(W, kStrip);
    hipLaunchKernelGGL(keypoint_strip_kernel, dim3(strips, Kp, R), dim3(kThreads), 0, as_stream(stream), rois, roi_stride, cls_or_null,
                       heat, stride_r, stride_k, stride_h, stride_w, Kp, ph, pw, H, W, (Best *)workspace);
    const int st = launch_status("keypoint_strip_kernel");
    if (st) return st;
    hipLaunchKernelGGL(keypoint_pick_kernel, dim3(cdiv((long long)R * Kp, 256)), dim3(256), 0, as_stream(stream),
                       (const Best *)workspace, R * Kp, strips, W, out);
    return launch_status("keypoint_pick_kernel");
}
