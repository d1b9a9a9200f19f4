// mask_resample.h -- Pillow's ImagingResample coefficients for a mode-F image with the default filter since Pillow 7 (BICUBIC,
// a = -0.5), shared by the paste (mask_ops.hip) and the resize to the original image size (mask_rescale.hip).  Every operation is one
// IEEE double operation per source operator: the files that include this are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace scda {

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

// the taps [*lo, *hi) of output sample xx of an axis n_in -> n_out, without their weights (equal sizes: the sample itself)
__device__ inline void axis_range(int n_in, int n_out, int xx, int *lo, int *hi) {
    if (n_in == n_out) {
        *lo = xx; *hi = xx + 1;
        return;
    }
    const double scale = (double)n_in / n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    *lo = xmin; *hi = xmax > xmin ? xmax : xmin;
}

// Pillow's precompute_coeffs for ONE output sample xx of an axis n_in -> n_out: first tap and tap count, normalised weights into w[]
// (equal sizes: Pillow skips the pass -- one tap of weight 1 reproduces the sample)
__device__ inline void axis_taps(int n_in, int n_out, int xx, int ks, int *first, int *count, double *w) {
    if (n_in == n_out) {
        *first = xx; *count = 1; w[0] = 1.0;
        return;
    }
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
    for (int k = 0; k < n; ++k) {
        const double v = bicubic((k + xmin - center + 0.5) * ss);
        w[k] = v;
        ww += v;
    }
    if (ww != 0.0)
        for (int k = 0; k < n; ++k) w[k] /= ww;
    *first = xmin; *count = n;
}

// float32 -> int as Python's int(): towards zero; what does not fit an int makes the RoI empty
__device__ inline bool trunc_ok(float v, int *out) {
    if (!(v > -5.0e8f && v < 5.0e8f)) return false;
    *out = (int)v;
    return true;
}

}  // namespace scda
