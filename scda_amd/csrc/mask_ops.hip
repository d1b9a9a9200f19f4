// mask_ops.hip -- instance masks of the mask-branch detector on the device (gfx950): the detections' RoIs, the class plane of
// each RoI's mask logits, and functions/mask.py:21-49 (`predict_masks`: the plane resized to the RoI by Pillow, pasted into the image).
//
// The resize is Pillow's ImagingResample on a mode-F image with its default filter since Pillow 7 (BICUBIC, a = -0.5, support 2):
// a horizontal pass into a float32 intermediate, then a vertical pass; per output sample the double weights are normalised by their
// left-to-right sum and the sample is (float) of the left-to-right double sum of (double)pixel * weight.  Every operation below is one
// IEEE operation per source operator (compiled with -ffp-contract=off), which makes the result Pillow's bit for bit; the rule is
// stated in include/scda_ops.h and restated in numpy by tests/test_mask_infer_rules.py.
#include "eval_prims.h"
#include "mask_resample.h"      // RoiWindow, AxisTable, horizontal_pass

namespace {
using namespace scda;

constexpr int kMaxIn = 32;                      // largest plane side (the mask head gives 28; the golden cases use 14)
constexpr int kStrip = 128;                     // image columns per workgroup
constexpr int kRows = 64;                       // image rows per vertical-table refill
constexpr int kThreads = kResampleThreads;
constexpr int kTmpStride = kStrip + kStrip / 32;    // room for the bit form's one-in-32 padding
constexpr int kTaps = 5;                        // table room per sample: an up-scaled axis has 5 taps; a down-scaled one of <= 32 fits too

template <bool BITS> __device__ inline int tmp_col(int x) { return BITS ? x + (x >> 5) : x; }

// grid (column strips, R), 256 threads.  A workgroup owns columns [c0, c0 + 128) of RoI r's plane and writes EVERY row of them.
// LDS: 4 KB plane + 16.5 KB horizontal pass + 6 KB and 3 KB tables = 29.5 KB.
template <bool BITS>
__global__ __launch_bounds__(kThreads) void mask_paste_kernel(const float *__restrict__ rois, int roi_stride, const int *__restrict__ cls,
                                                              const float *__restrict__ planes, int ph, int pw, int H, int W, int Wd,
                                                              float threshold, int vec4, void *__restrict__ out_) {
    __shared__ float plane[kMaxIn * kMaxIn];
    __shared__ __align__(16) float tmp[kMaxIn * kTmpStride];       // the horizontal pass: [ph][this strip's columns]
    __shared__ AxisTable<kStrip, kTaps>::Lds hlds;
    __shared__ AxisTable<kRows, kTaps>::Lds vlds;
    AxisTable<kStrip, kTaps> htab(hlds);
    AxisTable<kRows, kTaps> vtab(vlds);
    static_assert(htab.holds(kMaxIn) && vtab.holds(kMaxIn), "a down-scaled axis of the largest plane fits both tables");
    const int r = blockIdx.y, c0 = blockIdx.x * kStrip, t = threadIdx.x;
    // columns [ca, cb) of this strip and rows [ya, yb) of the plane lie inside the window (uniform over the workgroup)
    const RoiWindow win = read_roi_window(rois, roi_stride, cls, r);
    int ca = 0, cb = 0, ya = 0, yb = 0;
    const bool live = win.live && win.clip_x(c0, min(W, c0 + kStrip), &ca, &cb) && win.clip_y(0, H, &ya, &yb);
    if (live) {
        for (int i = t; i < ph * pw; i += kThreads) plane[i] = planes[(size_t)r * ph * pw + i];
        htab.fill(pw, win.w, ca - win.x1, cb - ca);
        __syncthreads();
        horizontal_pass(plane, pw, ph, htab, cb - ca, tmp, kTmpStride, [=](int xa) { return tmp_col<BITS>(ca - c0 + xa); });
    }
    for (int ybase = 0; ybase < H; ybase += kRows) {
        const bool hit = live && ybase < yb && ybase + kRows > ya;
        const int tv0 = ya > ybase ? ya : ybase;               // the first table row of this refill
        __syncthreads();                                       // tmp is complete / the previous refill has been read
        if (hit) vtab.fill(ph, win.h, tv0 - win.y1, min(yb, ybase + kRows) - tv0);
        __syncthreads();
        if (BITS) {
            // one row and one 32-column word per thread
            const int y = ybase + (t >> 2), word = (c0 >> 5) + (t & 3);
            if (y < H && word < Wd) {
                // outside the window the plane is 0.0f: its bit is (0.0f >= threshold) like any other value's; columns past W stay clear
                const int left = W - word * 32;
                unsigned int bits = 0.f >= threshold ? (left >= 32 ? 0xffffffffu : (1u << left) - 1u) : 0u;
                if (hit && y >= ya && y < yb) {
                    const int ty = y - tv0, n = vtab.count(ty);
                    const double *w = vtab.weights(ty);
                    const float *col = tmp + vtab.first(ty) * kTmpStride;
                    const int cl = word * 32 - c0;
                    for (int j = 0; j < 32; ++j) {
                        const int c = word * 32 + j;
                        if (c >= ca && c < cb)
                            bits = resample_dot(col + tmp_col<true>(cl + j), kTmpStride, w, n) >= threshold ? bits | (1u << j) : bits & ~(1u << j);
                    }
                }
                ((unsigned int *)out_)[((size_t)r * H + y) * Wd + word] = bits;
            }
        } else {
            // four adjacent columns per thread, eight rows per step
            const int cl = (t & 31) * 4, c = c0 + cl;
            float *out = (float *)out_;
            for (int y = ybase + (t >> 5); y < min(ybase + kRows, H); y += kThreads / 32) {
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (hit && y >= ya && y < yb && c < cb && c + 3 >= ca) {
                    const int ty = y - tv0;
                    float s[4];                                // (columns outside the window read what LDS holds and are dropped below)
                    resample_dot(tmp + vtab.first(ty) * kTmpStride + cl, kTmpStride, vtab.weights(ty), vtab.count(ty), s);
                    for (int q = 0; q < 4; ++q)
                        if (c + q >= ca && c + q < cb) v[q] = s[q];
                }
                float *dst = out + ((size_t)r * H + y) * W + c;
                if (vec4 && c + 3 < W) {
                    *(float4 *)dst = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    for (int q = 0; q < 4; ++q)
                        if (c + q < W) dst[q] = v[q];
                }
            }
        }
    }
}

__global__ void det_rois_kernel(const float *__restrict__ det, const int *__restrict__ counts, int B, int top_n, float *__restrict__ rois,
                                int *__restrict__ cls) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * top_n) return;
    const int b = i / top_n, j = i - b * top_n;
    const float *d = det + (size_t)i * 7;
    const bool real = j < counts[b];
    float *o = rois + (size_t)i * 5;
    o[0] = (float)b;
    for (int q = 1; q < 5; ++q) o[q] = real ? d[q] : 0.f;
    cls[i] = real ? (int)d[6] : -1;
}

// sigmoid(x) = 1 / (1 + e) with e = the correctly rounded float32 exp(-x) (float64 exp rounded once) and float32 IEEE add and divide
__global__ void mask_select_kernel(const float *__restrict__ logits, long long sr, long long sc, long long sh, long long sw,
                                   const int *__restrict__ cls, int R, int C, int ph, int pw, int sigmoid, float *__restrict__ out) {
    const long long n = (long long)R * ph * pw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % pw), y = (int)((i / pw) % ph), r = (int)(i / ((long long)ph * pw));
        const int c = cls[r];
        float v = 0.f;
        if (c >= 0 && c < C) {
            v = logits[r * sr + c * sc + y * sh + x * sw];
            if (sigmoid) v = 1.0f / (1.0f + (float)exp(-(double)v));
        }
        out[i] = v;
    }
}

}  // namespace

SCDA_API int scda_det_rois_hip(const float *detections, const int *detection_counts, int B, int top_n, float *rois5, int *cls,
                               void *stream) {
    SCDA_CHECK_ARGS(detections && detection_counts && rois5 && cls && B > 0 && top_n > 0 && (long long)B * top_n < 0x7fffffffLL,
                    "scda_det_rois_hip")
    hipLaunchKernelGGL(det_rois_kernel, dim3(cdiv((long long)B * top_n, 256)), dim3(256), 0, as_stream(stream), detections,
                       detection_counts, B, top_n, rois5, cls);
    return launch_status("det_rois_kernel");
}

SCDA_API int scda_mask_select_hip(const float *logits, long long stride_r, long long stride_c, long long stride_h, long long stride_w,
                                  const int *cls, int R, int C, int ph, int pw, int sigmoid, float *out, void *stream) {
    SCDA_CHECK_ARGS(logits && cls && out && R > 0 && C > 0 && ph > 0 && pw > 0 && stride_r >= 0 && stride_c >= 0 && stride_h >= 0 &&
                    stride_w >= 0, "scda_mask_select_hip")
    hipLaunchKernelGGL(mask_select_kernel, dim3(ew_grid((long long)R * ph * pw)), dim3(256), 0, as_stream(stream), logits, stride_r,
                       stride_c, stride_h, stride_w, cls, R, C, ph, pw, sigmoid, out);
    return launch_status("mask_select_kernel");
}

SCDA_API int scda_mask_paste_hip(const float *rois, int roi_stride, const int *cls_or_null, const float *planes, int R, int ph, int pw,
                                 int H, int W, int packed, float threshold, void *out, void *stream) {
    SCDA_CHECK_ARGS(rois && planes && out && R > 0 && R <= 65535 && roi_stride >= 5 && ph > 0 && pw > 0 && ph <= kMaxIn && pw <= kMaxIn &&
                    H > 0 && W > 0, "scda_mask_paste_hip")
    const int Wd = (W + 31) / 32;
    const dim3 grid(cdiv(W, kStrip), R);
    if (packed) {
        hipLaunchKernelGGL(mask_paste_kernel<true>, grid, dim3(kThreads), 0, as_stream(stream), rois, roi_stride, cls_or_null, planes, ph,
                           pw, H, W, Wd, threshold, 0, out);
    } else {
        const int vec4 = W % 4 == 0 && (uintptr_t)out % 16 == 0;
        hipLaunchKernelGGL(mask_paste_kernel<false>, grid, dim3(kThreads), 0, as_stream(stream), rois, roi_stride, cls_or_null, planes,
                           ph, pw, H, W, Wd, threshold, vec4, out);
    }
    return launch_status("mask_paste_kernel");
}
