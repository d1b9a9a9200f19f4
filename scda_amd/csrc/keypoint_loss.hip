// keypoint_loss.hip -- training the keypoint branch (gfx950): the soft-max cross-entropy over the HW positions of each (RoI, keypoint)
// heat map, averaged over the counted pairs.  include/scda_ops.h states the definition and the target rule (both OUR choice: the
// reference's are in its missing models/mask_rcnn/mask_rcnn.py).
//
// What the class-count kernel of nn_ops.hip (softmax_ce_fwd_kernel: one workgroup for the call, one thread per row, a [R, C] probability
// tensor, a contiguous [R, C] input) cannot do at C = 56 * 56 = 3136 and 64 * 17 = 1088 rows:
//   * one workgroup per map; the map is read from memory ONCE, coalesced, and stays in registers (HW <= 4096 = 16 floats per thread)
//     between the max pass and the sum pass; a map whose target is -1 is not read at all;
//   * planes are addressed by the element strides of R and Kp, so the keypoint head's transposed channel-major view goes in as it is,
//     and the backward writes the gradient in the same layout;
//   * (max, log-sum) per map is all the backward needs: no probability tensor;
//   * the sum over maps is a second, single-workgroup launch over row_loss in a fixed order (block_sum of common.h): no float atomics,
//     the same bytes on every launch.
#include <float.h>

#include "eval_prims.h"         // SCDA_CHECK_ARGS

namespace {
using namespace scda;

constexpr int kThreads = 256;
constexpr int kMaxHW = 4096;                    // the decode's 64 x 64 limit
constexpr int kPer = kMaxHW / kThreads;         // map elements per thread, in registers

__device__ inline bool counted(int tgt, int HW) { return tgt >= 0 && tgt < HW; }

// grid (R * Kp), 256 threads: map m = r * Kp + k -> stats[2m .. 2m+1] = (max, log sum exp(x - max)), row_loss[m]
__global__ __launch_bounds__(kThreads) void keypoint_ce_fwd_kernel(const float *__restrict__ heat, long long sr, long long sk, int Kp, int HW,
                                                                   const int *__restrict__ targets, float *__restrict__ stats,
                                                                   float *__restrict__ row_loss) {
    __shared__ float red[16];
    __shared__ float at_target;
    const int m = blockIdx.x, t = threadIdx.x;
    const int tgt = targets[m];                                    // uniform over the workgroup
    if (!counted(tgt, HW)) {
        if (t == 0) { stats[2 * (size_t)m] = 0.f; stats[2 * (size_t)m + 1] = 0.f; row_loss[m] = 0.f; }
        return;
    }
    const int r = m / Kp, k = m - r * Kp;
    const float *x = heat + r * sr + k * sk;
    float v[kPer];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = t + j * kThreads;
        v[j] = i < HW ? x[i] : -INFINITY;
        mx = fmaxf(mx, v[j]);
        if (i == tgt) at_target = v[j];                            // one thread of the workgroup; read behind block_max's barriers
    }
    mx = block_max(mx, red);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kPer; ++j)
        if (t + j * kThreads < HW) s += expf(v[j] - mx);
    s = block_sum(s, red);
    if (t == 0) {
        const float ls = logf(s);
        stats[2 * (size_t)m] = mx;
        stats[2 * (size_t)m + 1] = ls;
        row_loss[m] = (mx - at_target) + ls;
    }
}

// one workgroup: out2 = (sum of row_loss over the counted maps / their number, that number), (0, 0) when there is none.  Each thread
// adds its maps in index order, block_sum joins the threads in a fixed tree.
__global__ __launch_bounds__(kThreads) void keypoint_ce_mean_kernel(const float *__restrict__ row_loss, const int *__restrict__ targets, int n,
                                                                    int HW, float *__restrict__ out2) {
    __shared__ float red[16];
    float s = 0.f, c = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads)
        if (counted(targets[i], HW)) { s += row_loss[i]; c += 1.f; }
    s = block_sum(s, red);
    c = block_sum(c, red);
    if (threadIdx.x == 0) { out2[0] = c > 0.f ? s / c : 0.f; out2[1] = c; }
}

// grid (R * Kp), 256 threads: the plane of map m in dheat <- (softmax - onehot) * g / count, or zeros for an uncounted map
__global__ __launch_bounds__(kThreads) void keypoint_ce_bwd_kernel(const float *__restrict__ heat, long long sr, long long sk, int Kp, int HW,
                                                                   const int *__restrict__ targets, const float *__restrict__ stats,
                                                                   const float *__restrict__ out2, const float *__restrict__ g,
                                                                   float *__restrict__ dheat, long long dsr, long long dsk) {
    const int m = blockIdx.x, t = threadIdx.x;
    const int r = m / Kp, k = m - r * Kp;
    float *d = dheat + r * dsr + k * dsk;
    const int tgt = targets[m];
    if (!counted(tgt, HW)) {
        for (int i = t; i < HW; i += kThreads) d[i] = 0.f;
        return;
    }
    const float *x = heat + r * sr + k * sk;
    const float scale = g[0] / out2[1];                            // this map is counted: out2[1] >= 1
    const float mx = stats[2 * (size_t)m], ls = stats[2 * (size_t)m + 1];
    for (int i = t; i < HW; i += kThreads) d[i] = (expf((x[i] - mx) - ls) - (i == tgt ? 1.f : 0.f)) * scale;
}

bool shape_ok(long long stride_r, long long stride_k, int R, int Kp, int HW) {
    return R > 0 && Kp > 0 && HW >= 1 && HW <= kMaxHW && (long long)R * Kp < (1LL << 24) && stride_r >= 0 && stride_k >= 0;
}

}  // namespace

SCDA_API int scda_keypoint_ce_fwd_hip(const float *heat, long long stride_r, long long stride_k, int R, int Kp, int HW, const int *targets,
                                      float *stats, float *row_loss, float *out2, void *stream) {
    SCDA_CHECK_ARGS(heat && targets && stats && row_loss && out2 && shape_ok(stride_r, stride_k, R, Kp, HW), "scda_keypoint_ce_fwd_hip")
    hipLaunchKernelGGL(keypoint_ce_fwd_kernel, dim3(R * Kp), dim3(kThreads), 0, as_stream(stream), heat, stride_r, stride_k, Kp, HW,
                       targets, stats, row_loss);
    const int st = launch_status("keypoint_ce_fwd_kernel");
    if (st) return st;
    hipLaunchKernelGGL(keypoint_ce_mean_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), (const float *)row_loss, targets, R * Kp, HW,
                       out2);
    return launch_status("keypoint_ce_mean_kernel");
}

SCDA_API int scda_keypoint_ce_bwd_hip(const float *heat, long long stride_r, long long stride_k, int R, int Kp, int HW, const int *targets,
                                      const float *stats, const float *out2, const float *grad_scalar, float *dheat, long long dstride_r,
                                      long long dstride_k, void *stream) {
    SCDA_CHECK_ARGS(heat && targets && stats && out2 && grad_scalar && dheat && shape_ok(stride_r, stride_k, R, Kp, HW) &&
                    dstride_r >= 0 && dstride_k >= 0, "scda_keypoint_ce_bwd_hip")
    hipLaunchKernelGGL(keypoint_ce_bwd_kernel, dim3(R * Kp), dim3(kThreads), 0, as_stream(stream), heat, stride_r, stride_k, Kp, HW,
                       targets, stats, out2, grad_scalar, dheat, dstride_r, dstride_k);
    return launch_status("keypoint_ce_bwd_kernel");
}
