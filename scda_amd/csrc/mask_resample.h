// mask_resample.h -- "resize a small plane to its RoI window as Pillow >= 7 resizes a mode-F image (BICUBIC, a = -0.5), bit for bit",
// stated once for the paste (mask_ops.hip), the resize to the original image size (mask_rescale.hip) and the keypoint decode
// (keypoint_ops.hip): Pillow's ImagingResample coefficients, the RoI window, the sample's dot product, the table of an axis' taps in LDS
// and the horizontal pass.  Every operation is one IEEE double operation per source operator: the files that include this are compiled
// with -ffp-contract=off.  All of it is device code for workgroups of kResampleThreads threads.
//
// Tables.  A table has room for SAMPLES * TAPS weights.  A run of samples whose normalised weights fit (count * ksize of them: always
// for an up-scaled or equal axis, which has at most 5 taps per sample, and for a down-scaled axis of a small plane, which has few
// samples) keeps them in LDS.  Only a table declared with RECOMPUTE (the vertical one of the keypoint kernel, whose planes go up to
// 64 x 64) can meet a run that does not fit: it then keeps per sample the first tap, the tap count and the weights' sum, and the weight
// of a tap is recomputed where it is used, bicubic(.) / sum: the same IEEE operations on the same operands in the same order as the
// tabulated weight, so the same bits.
#pragma once
#include "common.h"

namespace scda {

constexpr int kResampleThreads = 256;

__device__ inline double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// the table stride of an axis n_in -> n_out: Pillow's ksize = ceil(support) * 2 + 1, never more than the n_in taps a sample can have
__device__ inline int axis_ksize(int n_in, int n_out) {
    if (n_in == n_out) return 1;
    double fs = (double)n_in / n_out;
    if (fs < 1.0) fs = 1.0;
    const int ks = (int)ceil(2.0 * fs) * 2 + 1;
    return ks < n_in ? ks : n_in;
}

// Pillow's precompute_coeffs bounds for ONE output sample xx of an axis n_in -> n_out, n_in != n_out: the taps [first, first + count),
// at most ks of them, and what their raw weights bicubic((k + first - center + 0.5) * ss) are computed from
struct AxisSpan { double center, ss; int first, count; };

__device__ inline AxisSpan axis_span(int n_in, int n_out, int xx, int ks) {
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
    return {center, ss, xmin, n};
}

__device__ inline double span_raw(const AxisSpan &a, int k) { return bicubic((k + a.first - a.center + 0.5) * a.ss); }

// the left-to-right sum of a sample's raw weights
__device__ inline double span_sum(const AxisSpan &a) {
    double ww = 0.0;
    for (int k = 0; k < a.count; ++k) ww += span_raw(a, k);
    return ww;
}

// tap k's normalised weight, given that sum
__device__ inline double span_weight(const AxisSpan &a, int k, double sum) {
    double w = span_raw(a, k);
    if (sum != 0.0) w /= sum;
    return w;
}

// the taps [*lo, *hi) of output sample xx of an axis n_in -> n_out, without their weights (equal sizes: the sample itself)
__device__ inline void axis_range(int n_in, int n_out, int xx, int *lo, int *hi) {
    if (n_in == n_out) {
        *lo = xx; *hi = xx + 1;
        return;
    }
    const AxisSpan a = axis_span(n_in, n_out, xx, n_in);
    *lo = a.first; *hi = a.first + a.count;
}

// first tap and tap count of output sample xx, normalised weights into w[] (equal sizes: Pillow skips the pass -- one tap of weight 1
// reproduces the sample)
__device__ inline void axis_taps(int n_in, int n_out, int xx, int ks, int *first, int *count, double *w) {
    if (n_in == n_out) {
        *first = xx; *count = 1; w[0] = 1.0;
        return;
    }
    const AxisSpan a = axis_span(n_in, n_out, xx, ks);
    double ww = 0.0;
    for (int k = 0; k < a.count; ++k) {
        const double v = span_raw(a, k);
        w[k] = v;
        ww += v;
    }
    if (ww != 0.0)
        for (int k = 0; k < a.count; ++k) w[k] /= ww;
    *first = a.first; *count = a.count;
}

// float32 -> int as Python's int(): towards zero; what does not fit an int makes the RoI empty
__device__ inline bool trunc_ok(float v, int *out) {
    if (!(v > -5.0e8f && v < 5.0e8f)) return false;
    *out = (int)v;
    return true;
}

// ---- the window of RoI r = (b, x1, y1, x2, y2, ...): columns [x1, x1 + w), rows [y1, y1 + h) of the image.  Not live: a padding row
// (cls[r] < 0), a coordinate that is not finite or does not fit an int, x2 < x1 or y2 < y1 -- an empty mask.
struct RoiWindow {
    int x1, y1, w, h;
    bool live;
    // the part [*a, *b) of the window's columns / rows inside [lo, hi); false when there is none
    __device__ bool clip_x(int lo, int hi, int *a, int *b) const { return clip(x1, w, lo, hi, a, b); }
    __device__ bool clip_y(int lo, int hi, int *a, int *b) const { return clip(y1, h, lo, hi, a, b); }
    __device__ static bool clip(int at, int n, int lo, int hi, int *a, int *b) {
        *a = at > lo ? at : lo;
        *b = min(at + n, hi);
        return *a < *b;
    }
};

__device__ inline RoiWindow read_roi_window(const float *rois, int roi_stride, const int *cls, int r, bool live = true) {
    const float *roi = rois + (size_t)r * roi_stride;
    int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    live = live && !(cls && cls[r] < 0);
    live = trunc_ok(roi[1], &x1) && live;
    live = trunc_ok(roi[2], &y1) && live;
    live = trunc_ok(roi[3], &x2) && live;
    live = trunc_ok(roi[4], &y2) && live;
    RoiWindow win = {x1, y1, 0, 0, false};
    if (live) {
        win.w = x2 - x1 + 1; win.h = y2 - y1 + 1;
        win.live = win.w > 0 && win.h > 0;
    }
    return win;
}

// ---- one sample: (float) of the left-to-right double sum of (double)pixel * weight over the n taps src[0], src[stride], ...
__device__ inline float resample_dot(const float *src, int stride, const double *w, int n) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += (double)src[k * stride] * w[k];
    return (float)s;
}

// the same with the weights recomputed per tap from the sample's span and its weights' sum
__device__ inline float resample_dot(const float *src, int stride, const AxisSpan &a, double sum) {
    double s = 0.0;
    for (int k = 0; k < a.count; ++k) s += (double)src[k * stride] * span_weight(a, k, sum);
    return (float)s;
}

// four adjacent columns against one sample's weights (src 16-byte aligned, stride in floats)
__device__ inline void resample_dot(const float *src, int stride, const double *w, int n, float out[4]) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < n; ++k) {
        const float4 p = *(const float4 *)(src + k * stride);
        s[0] += (double)p.x * w[k]; s[1] += (double)p.y * w[k]; s[2] += (double)p.z * w[k]; s[3] += (double)p.w * w[k];
    }
    for (int q = 0; q < 4; ++q) out[q] = (float)s[q];
}

// ---- the taps of a run of at most SAMPLES consecutive output samples of one axis.  The arrays live in LDS (an AxisTable<..>::Lds
// declared __shared__ by the kernel); the table itself is a handle every thread holds: fill() sets its state, so EVERY thread of the
// workgroup calls fill(), with the same arguments, before it reads the table.
// RECOMPUTE = false: the kernel's limits guarantee that every run fits (the kernel asserts holds()), and only the tabulated form is
// compiled.
template <int SAMPLES, int TAPS, bool RECOMPUTE = false>
class AxisTable {
public:
    struct Lds {
        double w[SAMPLES * TAPS];       // tabulated: sample i's weights at w[i * ksize]; else its weights' raw sum at w[i]
        int first[SAMPLES], count[SAMPLES];
    };
    __device__ explicit AxisTable(Lds &lds) : lds_(lds) {}
    // every run of an axis from at most n_in samples fits: up-scaled, count <= SAMPLES samples of 5 taps; down-scaled, n_out samples
    // of ksize <= 4 n_in / n_out + 3 taps, fewer than 7 n_in weights
    static constexpr bool holds(int n_in) { return TAPS >= 5 && 7 * n_in <= SAMPLES * TAPS; }

    // samples [first_sample, first_sample + count) of the axis n_in -> n_out become entries 0 .. count - 1; block-strided -- SINGLE:
    // one pass, for a fill inside a latency-bound loop -- and the caller puts a barrier between this and the first read (and between
    // the last read and the next fill)
    template <bool SINGLE = false>
    __device__ void fill(int n_in, int n_out, int first_sample, int count) {
        static_assert(!SINGLE || SAMPLES <= kResampleThreads, "one pass needs a thread per sample");
        n_in_ = n_in; n_out_ = n_out; x0_ = first_sample; ks_ = axis_ksize(n_in, n_out);
        tabulated_ = !RECOMPUTE || count * ks_ <= SAMPLES * TAPS;
        for (int i = threadIdx.x; i < count; i += kResampleThreads) {
            if (tabulated_) {
                // (memory safety only: beyond what holds() covers the taps are cut, nothing is overrun)
                const int room = SAMPLES * TAPS - i * ks_;
                axis_taps(n_in, n_out, x0_ + i, room < ks_ ? max(room, 0) : ks_, &lds_.first[i], &lds_.count[i], &lds_.w[i * ks_]);
            } else {
                const AxisSpan a = axis_span(n_in, n_out, x0_ + i, ks_);
                lds_.first[i] = a.first; lds_.count[i] = a.count; lds_.w[i] = span_sum(a);
            }
            if (SINGLE) break;
        }
    }
    __device__ int first(int i) const { return lds_.first[i]; }
    __device__ int count(int i) const { return lds_.count[i]; }
    // sample i's weights, for a consumer that reads them once for several lines
    __device__ const double *weights(int i) const {
        static_assert(!RECOMPUTE, "a table that may recompute has no weights to hand out");
        return lds_.w + i * ks_;
    }
    // sample i of the line whose tap first(i) is at src
    __device__ float dot(int i, const float *src, int stride) const {
        if (RECOMPUTE && !tabulated_) return resample_dot(src, stride, axis_span(n_in_, n_out_, x0_ + i, ks_), lds_.w[i]);
        return resample_dot(src, stride, lds_.w + i * ks_, lds_.count[i]);
    }

private:
    Lds &lds_;
    int n_in_ = 1, n_out_ = 1, x0_ = 0, ks_ = 1;
    bool tabulated_ = true;
};

// ---- the first pass, plane [ph][pw] -> tmp[row * tmp_stride + col_of(i)] for the na samples of `table`
template <class Table, class ColOf>
__device__ inline void horizontal_pass(const float *plane, int pw, int ph, const Table &table, int na, float *tmp, int tmp_stride,
                                       ColOf col_of) {
    for (int i = threadIdx.x; i < ph * na; i += kResampleThreads) {
        const int row = i / na, xa = i - row * na;
        tmp[row * tmp_stride + col_of(xa)] = table.dot(xa, plane + row * pw + table.first(xa), 1);
    }
}

}  // namespace scda
