// cluster_ops.hip -- the cluster-region generator on the device (functions/mask.py:183-237): sklearn 1.7.2's
// KMeans(n_clusters=k, random_state=0).fit on the RoI centres and the member lists in ONE launch of ONE workgroup
// (scda_kmeans_hip), and the gather of the cluster features (scda_cluster_gather_hip).  include/scda_ops.h states the rule.
//
// Arithmetic: float64 on the float32 centred points, one IEEE operation per source operator (-ffp-contract=off).  Every sum has
// a fixed order -- lane l of ONE wave adds elements l, l + 64, ... in turn, then the 64 partial sums meet in an xor butterfly
// (addition commutes, so all lanes hold the same bits) -- and there are no floating-point atomics: two runs are bit-identical,
// and tests/kmeans_np.py restates the same order.
#include "common.h"

namespace scda {

constexpr int kClusterCap = 1024;      // points: one per thread of the one workgroup
constexpr int kClusterMaxK = 8;        // 2 k sums of the M-step <= 16 waves
constexpr int kClusterMaxTrials = 4;   // 2 + int(ln 8)
constexpr int kClusterMaxIter = 300;

struct SeedDraws {
    double u[(kClusterMaxK - 1) * kClusterMaxTrials];   // [k-1][t]
};

__device__ inline double wave_sum64(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, kWave);
    return v;
}

// the fixed-order sum of a[0..n) by one whole wave
__device__ inline double lds_sum64(const double *a, int n, int lane) {
    double acc = 0.0;
    for (int i = lane; i < n; i += kWave) acc = acc + a[i];
    return wave_sum64(acc);
}

__device__ inline double sqdist(double x, double y, double cx, double cy) {
    const double dx = x - cx, dy = y - cy;
    return dx * dx + dy * dy;
}

__global__ __launch_bounds__(kClusterCap) void kmeans_kernel(const float *rois, int roi_stride, int N, int k, int first, int trials,
                                                             SeedDraws draws, float *centres, int *labels, int *counts, int *members,
                                                             int *seed_index, int *n_iter_out, int *status_out) {
    __shared__ double sx[kClusterCap], sy[kClusterCap], sclose[kClusterCap], scum[kClusterCap];
    __shared__ int slab[kClusterCap];
    __shared__ double sred[2 * kClusterMaxK], spots[kClusterMaxTrials], sshift[kClusterMaxK], scx[kClusterMaxK], scy[kClusterMaxK];
    __shared__ double spot;
    __shared__ int scount[kClusterMaxK], scand[kClusterMaxTrials], sseed[kClusterMaxK];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (N < 1 || N > kClusterCap || k < 1 || k > kClusterMaxK || k > N || first < 0 || first >= N || trials < 1 ||
        trials > kClusterMaxTrials) {                                     // (uniform: every thread leaves)
        if (tid == 0) { *status_out = 2; *n_iter_out = 0; }
        return;
    }
    const bool live = tid < N;
    // 1. points: the RoI centres in float32
    float xf = 0.f, yf = 0.f;
    if (live) {
        const float *r = rois + (size_t)tid * roi_stride;
        xf = (r[3] + r[1]) / 2.0f;
        yf = (r[4] + r[2]) / 2.0f;
        sx[tid] = (double)xf;
        sy[tid] = (double)yf;
    }
    __syncthreads();
    if (wave < 2) {
        const double s = lds_sum64(wave ? sy : sx, N, lane);
        if (lane == 0) sred[wave] = s;
    }
    __syncthreads();
    // 2. tolerance: 1e-4 * mean of the two variances; 3. centring in float32
    const double mx = sred[0] / (double)N, my = sred[1] / (double)N;
    if (live) {
        const double d0 = (double)xf - mx, d1 = (double)yf - my;
        sclose[tid] = d0 * d0;
        scum[tid] = d1 * d1;
    }
    __syncthreads();
    if (wave < 2) {
        const double s = lds_sum64(wave ? scum : sclose, N, lane);
        if (lane == 0) sred[2 + wave] = s;
    }
    __syncthreads();
    const double tol_abs = 1e-4 * ((sred[2] / (double)N + sred[3] / (double)N) / 2.0);
    if (!(__builtin_isfinite(mx) && __builtin_isfinite(my) && __builtin_isfinite(tol_abs))) {      // (uniform: all read the same sred)
        if (tid < k) counts[tid] = 0;            // a NaN or infinite coordinate: sklearn raises on it, so the host path answers
        if (tid == 0) { *status_out = 4; *n_iter_out = 0; }
        return;
    }
    const float mxf = (float)mx, myf = (float)my;
    const double x = (double)(xf - mxf), y = (double)(yf - myf);
    if (live) { sx[tid] = x; sy[tid] = y; }
    __syncthreads();
    // 4. k-means++ seeding
    double closest = sqdist(x, y, sx[first], sy[first]);
    if (live) sclose[tid] = closest;
    if (tid == 0) sseed[0] = first;
    __syncthreads();
    if (wave == 0) {
        const double s = lds_sum64(sclose, N, lane);
        if (lane == 0) spot = s;
    }
    for (int c = 1; c < k; ++c) {
        __syncthreads();                         // sclose and spot of the round before (or of the first seed) are written
        if (tid == 0) {                          // the sequential float64 cumsum (stable_cumsum)
            double run = 0.0;
            for (int i = 0; i < N; ++i) { run = run + sclose[i]; scum[i] = run; }
        }
        __syncthreads();
        if (tid < trials) {                      // np.searchsorted(cum, u * pot) (side 'left'), clipped to N - 1
            const double v = draws.u[(c - 1) * trials + tid] * spot;
            int lo = 0, hi = N;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (scum[mid] < v) lo = mid + 1; else hi = mid;
            }
            scand[tid] = lo < N - 1 ? lo : N - 1;
        }
        __syncthreads();
        if (wave < trials) {                     // the potential with each candidate added: one wave per candidate
            const int j = scand[wave];
            const double cx = sx[j], cy = sy[j];
            double acc = 0.0;
            for (int i = lane; i < N; i += kWave) acc = acc + fmin(sclose[i], sqdist(sx[i], sy[i], cx, cy));
            acc = wave_sum64(acc);
            if (lane == 0) spots[wave] = acc;
        }
        __syncthreads();
        int best = 0;
        for (int j = 1; j < trials; ++j)
            if (spots[j] < spots[best]) best = j;               // the first minimum
        const int pick = scand[best];
        const double pot = spots[best];
        closest = fmin(closest, sqdist(x, y, sx[pick], sy[pick]));
        if (live) sclose[tid] = closest;         // (the candidate waves finished reading sclose before the barrier above)
        if (tid == 0) { spot = pot; sseed[c] = pick; }
    }
    __syncthreads();
    if (tid < k) { scx[tid] = sx[sseed[tid]]; scy[tid] = sy[sseed[tid]]; }
    __syncthreads();
    // 5. Lloyd
    int old = -1, lab = 0, n_iter = kClusterMaxIter, status = 0;
    bool rerun = true;
    for (int it = 0; it < kClusterMaxIter; ++it) {
        double best = sqdist(x, y, scx[0], scy[0]);
        lab = 0;
        for (int c = 1; c < k; ++c) {
            const double d = sqdist(x, y, scx[c], scy[c]);
            if (d < best) { best = d; lab = c; }                // the first minimum
        }
        if (live) slab[tid] = lab;
        const int changed = __syncthreads_or(live && lab != old);
        if (wave < 2 * k) {                      // wave 2c sums cluster c's x and counts it, wave 2c + 1 sums its y
            const int c = wave >> 1;
            const double *src = (wave & 1) ? sy : sx;
            double acc = 0.0;
            int cnt = 0;
            for (int i = lane; i < N; i += kWave) {
                const bool in = slab[i] == c;
                acc = acc + (in ? src[i] : 0.0);
                cnt += in;
            }
            acc = wave_sum64(acc);
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s, kWave);
            if (lane == 0) {
                sred[wave] = acc;
                if (!(wave & 1)) scount[c] = cnt;
            }
        }
        __syncthreads();
        if (tid < k) {
            if (scount[tid] > 0) {
                const double nx = sred[2 * tid] / (double)scount[tid], ny = sred[2 * tid + 1] / (double)scount[tid];
                sshift[tid] = sqdist(nx, ny, scx[tid], scy[tid]);
                scx[tid] = nx;
                scy[tid] = ny;
            } else {
                sshift[tid] = 0.0;               // (an empty cluster ends the run below; its shift is never used)
            }
        }
        __syncthreads();
        bool empty = false;
        double shift = 0.0;
        for (int c = 0; c < k; ++c) {
            empty = empty || scount[c] == 0;
            shift = shift + sshift[c];
        }
        if (empty) { status = 1; break; }        // 6. sklearn relocates an empty cluster: not restated
        if (!changed) { n_iter = it + 1; rerun = false; break; }      // strict convergence: the means just computed stand
        if (shift <= tol_abs) { n_iter = it + 1; break; }
        old = lab;
    }
    if (status == 0 && rerun) {                  // the E-step against the final centres
        double best = sqdist(x, y, scx[0], scy[0]);
        lab = 0;
        for (int c = 1; c < k; ++c) {
            const double d = sqdist(x, y, scx[c], scy[c]);
            if (d < best) { best = d; lab = c; }
        }
        if (live) slab[tid] = lab;               // (two barriers since the M-step waves read slab)
    }
    __syncthreads();
    if (status != 0) {
        if (tid < k) counts[tid] = 0;
        if (tid == 0) { *status_out = status; *n_iter_out = 0; }
        return;
    }
    // 7. member lists: wave c compacts cluster c's indices in ascending order; the tail of the row is -1
    if (wave < k) {
        int base = 0;
        for (int i0 = 0; i0 < N; i0 += kWave) {
            const int i = i0 + lane;
            const bool in = i < N && slab[i] == wave;
            const unsigned long long mask = __ballot(in);
            if (in) members[(size_t)wave * N + base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
            base += __popcll(mask);
        }
        for (int i = base + lane; i < N; i += kWave) members[(size_t)wave * N + i] = -1;
        if (lane == 0) { counts[wave] = base; scount[wave] = base; }
    }
    if (live) labels[tid] = lab;
    if (tid < k) {
        centres[2 * tid] = (float)scx[tid] + mxf;
        centres[2 * tid + 1] = (float)scy[tid] + myf;
        seed_index[tid] = sseed[tid];
    }
    __syncthreads();
    if (tid == 0) {
        bool empty = false;                      // finally empty (possible after the re-run E-step): the host path raises as the reference does
        for (int c = 0; c < k; ++c) empty = empty || scount[c] == 0;
        *status_out = empty ? 1 : 0;
        *n_iter_out = n_iter;
    }
}

// out[c, j, :] = feats[row(c, j), :]: one workgroup per output row, 16 bytes per lane and access
template <bool VEC>
__global__ __launch_bounds__(256) void cluster_gather_kernel(const float *feats, long long feat_stride, int N, int F, const int *members,
                                                             const int *counts, const int *picks, int threshold, float *out) {
    const int row = blockIdx.x, c = row / threshold, j = row - c * threshold;
    const int cnt = counts[c];
    int src = -1;
    if (cnt >= threshold) {
        if (j < N) src = members[(size_t)c * N + j];
    } else if (picks) {
        const int p = picks[row];
        if (p >= 0 && p < cnt && p < N) src = members[(size_t)c * N + p];
    }
    const bool ok = src >= 0 && src < N;          // anything else (an empty cluster, a pick outside the list): a row of zeros
    float *dst = out + (size_t)row * F;
    const float *from = feats + (size_t)(ok ? src : 0) * feat_stride;
    if (VEC) {
        const float4 *f4 = reinterpret_cast<const float4 *>(from);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int i = threadIdx.x; i < F / 4; i += blockDim.x) d4[i] = ok ? f4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int i = threadIdx.x; i < F; i += blockDim.x) dst[i] = ok ? from[i] : 0.f;
    }
}

}  // namespace scda

using namespace scda;

SCDA_API int scda_kmeans_capacity(void) { return kClusterCap; }

SCDA_API int scda_kmeans_hip(const float *rois, int roi_stride, int N, int k, int first_index, const double *uniforms_host, int trials,
                             float *centres, int *labels, int *counts, int *members, int *seed_index, int *n_iter, int *status,
                             void *stream) {
    if (!(rois && centres && labels && counts && members && seed_index && n_iter && status && roi_stride >= 5 && (k <= 1 || uniforms_host))) {
        set_error("scda_kmeans_hip: bad arguments");
        return SCDA_EINVAL;
    }
    SeedDraws draws = {};
    if (k >= 2 && k <= kClusterMaxK && trials >= 1 && trials <= kClusterMaxTrials)      // (anything else: the kernel raises status bit 1)
        for (int i = 0; i < (k - 1) * trials; ++i) draws.u[i] = uniforms_host[i];
    hipLaunchKernelGGL(kmeans_kernel, dim3(1), dim3(kClusterCap), 0, as_stream(stream), rois, roi_stride, N, k, first_index, trials, draws,
                       centres, labels, counts, members, seed_index, n_iter, status);
    return launch_status("kmeans_kernel");
}

SCDA_API int scda_cluster_gather_hip(const float *feats, long long feat_stride, int N, int F, const int *members, const int *counts,
                                     const int *picks_or_null, int k, int threshold, float *out, void *stream) {
    if (!(feats && members && counts && out && N > 0 && F > 0 && feat_stride >= F && k > 0 && threshold > 0 &&
          (long long)k * threshold <= 0x7fffffffLL)) {
        set_error("scda_cluster_gather_hip: bad arguments");
        return SCDA_EINVAL;
    }
    const bool vec = F % 4 == 0 && feat_stride % 4 == 0 && ((uintptr_t)feats % 16 == 0) && ((uintptr_t)out % 16 == 0);
    if (vec)
        hipLaunchKernelGGL(cluster_gather_kernel<true>, dim3(k * threshold), dim3(256), 0, as_stream(stream), feats, feat_stride, N, F,
                           members, counts, picks_or_null, threshold, out);
    else
        hipLaunchKernelGGL(cluster_gather_kernel<false>, dim3(k * threshold), dim3(256), 0, as_stream(stream), feats, feat_stride, N, F,
                           members, counts, picks_or_null, threshold, out);
    return launch_status("cluster_gather_kernel");
}
