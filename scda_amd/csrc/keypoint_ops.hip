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
// LDS.  Planes go up to 64 x 64, so a down-scaled axis (fewer than 64 output samples, a small window) has up to 64 taps per sample:
// tabulating it would take 63 * 64 doubles = 32 KB per axis, 113 KB with the plane and the horizontal pass -- one workgroup per CU.
// mask_resample.h's tables keep the weights of a run of samples only when they fit (5 per sample on average), and otherwise per sample
// the first tap, the tap count and the weights' sum.  16 KB plane + 32 KB horizontal pass + 6 KB and 3 KB tables = 57.0 KB.
#include "eval_prims.h"
#include "mask_resample.h"      // RoiWindow, AxisTable, horizontal_pass

#include <climits>

namespace {
using namespace scda;

constexpr int kMaxIn = 64;                      // largest plane side (the keypoint head gives 56)
constexpr int kStrip = 128;                     // image columns per workgroup
constexpr int kRows = 64;                       // window rows per vertical-table refill
constexpr int kThreads = kResampleThreads;
constexpr int kTaps = 5;                        // table room per sample: an up-scaled or equal axis has 5 taps (mask_resample.h)

struct Best { float v; int at; };               // a resized value and its position y * W + x in the image; INT_MAX: none yet

// np.argmax's order on (value, row-major position): a wins against b
__device__ inline bool better(float av, int aat, float bv, int bat) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (an || av == bv) return aat < bat;
    return av > bv;
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
    __shared__ AxisTable<kStrip, kTaps>::Lds hlds;
    __shared__ AxisTable<kRows, kTaps, true>::Lds vlds;
    __shared__ Best wave_part[kThreads / 64];
    AxisTable<kStrip, kTaps> htab(hlds);
    AxisTable<kRows, kTaps, true> vtab(vlds);            // the one table a run may not fit: 64 rows down-scaled to more than 21
    static_assert(htab.holds(kMaxIn), "a down-scaled axis of the largest plane fits the horizontal table");
    const int r = blockIdx.z, k = blockIdx.y, c0 = blockIdx.x * kStrip, t = threadIdx.x;
    // columns [ca, cb) of this strip and rows [ya, yb) of the image lie inside the window (uniform over the workgroup)
    const RoiWindow win = read_roi_window(rois, roi_stride, cls, r);
    int ca = 0, cb = 0, ya = 0, yb = 0;
    const bool live = win.live && win.clip_x(c0, min(W, c0 + kStrip), &ca, &cb) && win.clip_y(0, H, &ya, &yb);
    Best best = {-INFINITY, INT_MAX};
    if (live) {
        const int na = cb - ca;                                    // 1 .. kStrip
        const float *src_plane = heat + r * sr + k * sk;
        for (int i = t; i < ph * pw; i += kThreads) {
            const int y = i / pw, x = i - y * pw;
            plane[i] = src_plane[y * sh + x * sw];
        }
        htab.fill(pw, win.w, ca - win.x1, na);
        __syncthreads();
        horizontal_pass(plane, pw, ph, htab, na, tmp, kStrip, [](int xa) { return xa; });
        // ---- the vertical pass over the visible rows, kRows at a time; nothing is stored but each thread's best
        for (int ybase = ya; ybase < yb; ybase += kRows) {
            const int nv = min(yb - ybase, kRows);
            __syncthreads();                                       // tmp is complete / the previous refill has been read
            vtab.fill(ph, win.h, ybase - win.y1, nv);
            __syncthreads();
            for (int i = t; i < nv * na; i += kThreads) {          // row-major over this refill's part of the strip
                const int ty = i / na, xa = i - ty * na;
                const float v = vtab.dot(ty, tmp + vtab.first(ty) * kStrip + xa, kStrip);
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
