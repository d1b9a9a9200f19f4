// mask_poly.hip -- COCO ground-truth masks on the device (gfx950): COCO.annToMask of datasets/pycocotools/coco.py, i.e. rleFrPoly, rleMerge
// (intersect = 0), frUncompressedRLE and rleDecode of datasets/pycocotools/common/maskApi.c, from polygon vertices / run counts to
// scda_mask_paste_hip's packed planes.  The rule is stated in include/scda_ops.h as a parity fill and restated in numpy by
// tests/mask_poly_np.py; it is integer work plus single IEEE double operations (this unit is built with -ffp-contract=off), so the planes
// are the reference's bit for bit.  The only atomics are integer XORs / adds, which commute: two runs give the same bytes.
//
// Every polygon and every RLE ("shape") owns one column-major toggle plane of h * w + 1 bits in the workspace.  The kernel boundary is
// the only ordering between the launches:
//
//   (memset)              the toggle planes and the areas
//   poly_toggle_kernel    one wave per polygon edge, lanes over its points: the point and its predecessor in closed form, one atomicXor
//   rle_toggle_kernel     one workgroup per RLE: prefix sums of the counts (block_scan256 of eval_prims.h), one atomicXor per run end
//   parity_scan_kernel    one workgroup per shape: prefix parity over the linear pixel sequence, in place
//   plane_write_kernel    per 32 x 32 block of an output plane: gathers the block's columns from every shape of the plane, ORs them,
//                         transposes to row-major words, writes every word of the plane and adds the popcount to the area
#include <limits.h>

#include "eval_prims.h"

namespace {
using namespace scda;

constexpr int kThreads = 256;                   // block_scan256 (eval_prims.h) is written for it
constexpr int kMaxCoord = 65535;

// the image size inside plane n; false for a plane index or a size out of range (such shapes are skipped: nothing is written out of bounds)
__device__ inline bool plane_size(const int *__restrict__ sizes, int N, int H, int Wd, int n, int *h, int *w) {
    if (n < 0 || n >= N) return false;
    *h = sizes[2 * n];
    *w = sizes[2 * n + 1];
    return *h >= 1 && *h <= H && *w >= 1 && *w <= 32 * Wd;
}

// the last p in [0, P) with first[p] <= v (first is non-decreasing)
__device__ inline int owner(const int *__restrict__ first, int P, int v) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// the first index of the non-decreasing a[0 .. n) whose value is >= key
__device__ inline int lower_bound(const int *__restrict__ a, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// x[j] = (int)(5 * xy[2j] + .5), y[j] likewise (maskApi.c:165-166); false for a coordinate that is not finite or beyond +-65535
__device__ inline bool vertex(const double *__restrict__ xy, int i, int *x, int *y) {
    const double scale = 5;
    const double a = xy[2 * (size_t)i], b = xy[2 * (size_t)i + 1];
    if (!(fabs(a) <= (double)kMaxCoord && fabs(b) <= (double)kMaxCoord)) return false;
    *x = (int)(scale * a + .5);
    *y = (int)(scale * b + .5);
    return true;
}

// one edge as maskApi.c:170-174 sets it up: the (possibly swapped) start, the number of points, the slope
struct Edge { int xs, ys, n; bool flip, along_x, point; double s; };

__device__ inline Edge make_edge(int xs, int ys, int xe, int ye) {
    Edge e;
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    e.flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (e.flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    e.xs = xs; e.ys = ys;
    e.n = max(dx, dy) + 1;
    e.along_x = dx >= dy;
    e.point = dx == 0 && dy == 0;
    e.s = e.point ? 0.0 : e.along_x ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
    return e;
}

// point d of the edge (maskApi.c:175-179)
__device__ inline void edge_point(const Edge &e, int d, int *u, int *v) {
    const int t = e.flip ? e.n - 1 - d : d;
    if (e.point) {
        // s = 0.0 / 0 is NaN, and (int)NaN is INT_MIN where the reference was compiled (a GPU conversion gives 0)
        *u = e.xs; *v = INT_MIN;
    } else if (e.along_x) {
        *u = t + e.xs; *v = (int)(e.ys + e.s * t + .5);
    } else {
        *v = t + e.ys; *u = (int)(e.xs + e.s * t + .5);
    }
}

// grid (ceil(V / 4)), 256 threads: wave -> edge (= the index of its first vertex), lanes over the edge's points
__global__ __launch_bounds__(kThreads) void poly_toggle_kernel(const double *__restrict__ xy, int V, const int *__restrict__ poly_first,
                                                               const int *__restrict__ poly_plane, int P, const int *__restrict__ sizes,
                                                               int N, int H, int Wd, size_t TW, uint32_t *__restrict__ tog) {
    const int e = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= V) return;
    const int p = owner(poly_first, P, e);
    const int a = poly_first[p], b = poly_first[p + 1];
    if (a < 0 || b > V || e < a || e >= b) return;
    int h, w;
    if (!plane_size(sizes, N, H, Wd, poly_plane[p], &h, &w)) return;
    const int j = e - a, k = b - a;
    int x0, y0, x1, y1, xp = 0, yp = 0;
    bool ok = vertex(xy, e, &x0, &y0);
    ok = vertex(xy, j + 1 < k ? e + 1 : a, &x1, &y1) && ok;                 // x[k] = x[0]
    if (j > 0) ok = vertex(xy, e - 1, &xp, &yp) && ok;
    if (!ok) return;
    const Edge ed = make_edge(x0, y0, x1, y1);
    // the predecessor of the edge's first point is the LAST POINT of the edge before, by the same formula (not the vertex itself:
    // (int)(negative + .5) truncates towards zero)
    int lu = 0, lv = 0;
    if (j > 0) {
        const Edge pe = make_edge(xp, yp, x0, y0);
        edge_point(pe, pe.n - 1, &lu, &lv);
    }
    uint32_t *T = tog + (size_t)p * TW;
    const double scale = 5;
    for (int d = lane; d < ed.n; d += kWave) {
        int uq, vq, up, vp;
        edge_point(ed, d, &uq, &vq);
        if (d > 0) edge_point(ed, d - 1, &up, &vp);
        else if (j > 0) { up = lu; vp = lv; }
        else continue;                                                      // the very first point has no predecessor
        if (uq == up) continue;
        double xd = (double)(uq < up ? uq : uq - 1);
        xd = (xd + .5) / scale - .5;
        if (floor(xd) != xd || xd < 0 || xd > w - 1) continue;
        double yd = (double)(vq < vp ? vq : vp);
        yd = (yd + .5) / scale - .5;
        if (yd < 0) yd = 0; else if (yd > h) yd = h;
        yd = ceil(yd);
        const uint32_t pos = (uint32_t)((int)xd * h + (int)yd);             // <= h * w
        atomicXor(&T[pos >> 5], 1u << (pos & 31));
    }
}

// grid (Q), 256 threads.  tog: the first RLE's toggle plane
__global__ __launch_bounds__(kThreads) void rle_toggle_kernel(const uint32_t *__restrict__ counts, int C, const int *__restrict__ rle_first,
                                                              const int *__restrict__ rle_plane, const int *__restrict__ sizes, int N,
                                                              int H, int Wd, size_t TW, uint32_t *__restrict__ tog) {
    __shared__ unsigned long long wave_sums[kThreads / kWave];
    const int q = blockIdx.x, t = threadIdx.x;
    const int a = rle_first[q], b = rle_first[q + 1];
    int h, w;
    if (a < 0 || b > C || a > b || !plane_size(sizes, N, H, Wd, rle_plane[q], &h, &w)) return;
    const unsigned long long hw = (unsigned long long)h * (unsigned long long)w;
    const int m = b - a;
    uint32_t *T = tog + (size_t)q * TW;
    unsigned long long base = 0;
    for (int i0 = 0; i0 < m; i0 += kThreads) {
        const int i = i0 + t;
        unsigned long long all;
        // run i ends at the running sum; the pixels behind the last run stay 0 (a last run of zeros toggles nothing); a sum beyond
        // h * w (refused by the host layer, the reference writes past its buffer there) is dropped
        const unsigned long long pos = base + block_scan256<unsigned long long>(i < m ? counts[a + i] : 0ull, wave_sums, Add(), base, &all);
        if (i < m && pos <= hw && (i < m - 1 || !(m & 1))) atomicXor(&T[pos >> 5], 1u << (pos & 31));
        base = all;
    }
}

__device__ inline uint32_t prefix_parity(uint32_t x) {
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
    return x;                                                               // bit i = parity of the bits 0 .. i
}

// grid (P + Q), 256 threads, 4 words per thread and round.  In place: bit i of a plane becomes the parity of the toggles at positions <= i
__global__ __launch_bounds__(kThreads) void parity_scan_kernel(const int *__restrict__ poly_plane, int P, const int *__restrict__ rle_plane,
                                                               const int *__restrict__ sizes, int N, int H, int Wd, size_t TW,
                                                               uint32_t *__restrict__ tog) {
    __shared__ uint32_t wave_par[kThreads / kWave];
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int h, w;
    if (!plane_size(sizes, N, H, Wd, s < P ? poly_plane[s] : rle_plane[s - P], &h, &w)) return;
    const int nw4 = (((h * w + 31) >> 5) + 3) >> 2;                          // uint4 groups that hold the pixels; <= TW / 4
    uint4 *T4 = (uint4 *)(tog + (size_t)s * TW);
    uint32_t carry = 0;                                                     // parity of everything before this round
    for (int i0 = 0; i0 < nw4; i0 += kThreads) {
        const int i = i0 + t;
        uint4 v = i < nw4 ? T4[i] : make_uint4(0u, 0u, 0u, 0u);
        v.x = prefix_parity(v.x);
        v.y = prefix_parity(v.y) ^ (0u - (v.x >> 31));
        v.z = prefix_parity(v.z) ^ (0u - (v.y >> 31));
        v.w = prefix_parity(v.w) ^ (0u - (v.z >> 31));
        const unsigned long long odd = __ballot(v.w >> 31);                 // threads whose four words hold an odd number of toggles
        const uint32_t in_wave = (uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u;
        __syncthreads();                                                    // the previous round's wave_par are read
        if (lane == 0) wave_par[wv] = (uint32_t)__popcll(odd) & 1u;
        __syncthreads();
        uint32_t before = carry, all = carry;
#pragma unroll
        for (int q = 0; q < kThreads / kWave; ++q) {
            if (q < wv) before ^= wave_par[q];
            all ^= wave_par[q];
        }
        const uint32_t inv = 0u - (before ^ in_wave);
        if (i < nw4) T4[i] = make_uint4(v.x ^ inv, v.y ^ inv, v.z ^ inv, v.w ^ inv);
        carry = all;
    }
}

// the 32 bits of a column-major plane from bit position pos on (the word behind the last one read lies inside the plane's TW words)
__device__ inline uint32_t bits_at(const uint32_t *__restrict__ T, uint32_t pos) {
    const uint32_t i = pos >> 5, sh = pos & 31;
    const uint32_t lo = T[i];
    return sh ? (lo >> sh) | (T[i + 1] << (32 - sh)) : lo;
}

// grid (ceil(nrb * Wd / 256), N), nrb = ceil(H / 32).  A thread owns the block (rows 32 rb .., word column wc) of output plane n;
// neighbouring threads own neighbouring row blocks, so that they read neighbouring words of a column
__global__ __launch_bounds__(kThreads) void plane_write_kernel(const int *__restrict__ poly_plane, int P, const int *__restrict__ rle_plane,
                                                               int Q, const int *__restrict__ sizes, int N, int H, int Wd, int nrb,
                                                               size_t TW, const uint32_t *__restrict__ tog, uint32_t *__restrict__ bits,
                                                               uint32_t *__restrict__ area) {
    __shared__ uint32_t red[kThreads / kWave];
    const int n = blockIdx.y, idx = blockIdx.x * kThreads + threadIdx.x;
    const bool active = idx < nrb * Wd;
    uint32_t set = 0;
    if (active) {
        const int wc = idx / nrb, rb = idx - wc * nrb, y0 = rb * 32;
        uint32_t col[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) col[j] = 0u;
        int h, w;
        if (plane_size(sizes, N, H, Wd, n, &h, &w) && y0 < h && 32 * wc < w) {
            const int nr = min(32, h - y0), nc = min(32, w - 32 * wc);
            const uint32_t rowmask = nr >= 32 ? 0xffffffffu : (1u << nr) - 1u;
            const uint32_t pos0 = (uint32_t)(32 * wc) * (uint32_t)h + (uint32_t)y0;
            // poly_plane and rle_plane are non-decreasing: the shapes of plane n are two contiguous ranges
            const int p1 = lower_bound(poly_plane, P, n + 1), q1 = lower_bound(rle_plane, Q, n + 1);
            for (int p = lower_bound(poly_plane, P, n); p < p1; ++p) {
                const uint32_t *T = tog + (size_t)p * TW;
#pragma unroll
                for (int j = 0; j < 32; ++j)
                    if (j < nc) col[j] |= bits_at(T, pos0 + (uint32_t)j * (uint32_t)h);
            }
            for (int q = lower_bound(rle_plane, Q, n); q < q1; ++q) {
                const uint32_t *T = tog + (size_t)(P + q) * TW;
#pragma unroll
                for (int j = 0; j < 32; ++j)
                    if (j < nc) col[j] |= bits_at(T, pos0 + (uint32_t)j * (uint32_t)h);
            }
#pragma unroll
            for (int j = 0; j < 32; ++j) col[j] &= rowmask;
            transpose32(col);                                               // col[i] = the word of row y0 + i
        }
        uint32_t *out = bits + ((size_t)n * H + y0) * Wd + wc;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            if (y0 + i < H) out[(size_t)i * Wd] = col[i];
            set += __popc(col[i]);
        }
    }
    if (!area) return;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) set += __shfl_xor(set, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = set;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < kThreads / kWave; ++q) set += red[q];
        if (set) atomicAdd(area + n, set);
    }
}

// words of one toggle plane: h * w + 1 bits, one word more for bits_at, a multiple of four for the uint4 scan
inline size_t toggle_words(int H, int Wd) { return (((size_t)H * Wd + 2) + 3) & ~(size_t)3; }

bool plane_ok(int N, int H, int Wd) {
    return N > 0 && N <= 65535 && H > 0 && H <= 65535 && Wd > 0 && (long long)H * Wd * 32 < 0x7fffffffLL;
}

}  // namespace

SCDA_API size_t scda_mask_frpoly_workspace_bytes(int P, int Q, int H, int Wd) {
    if (P < 0 || Q < 0 || !plane_ok(1, H, Wd)) return 0;
    const size_t bytes = ((size_t)P + Q) * toggle_words(H, Wd) * sizeof(uint32_t);
    return bytes ? bytes : 16;
}

SCDA_API int scda_mask_frpoly_hip(const double *xy, int V, const int *poly_first, const int *poly_plane, int P, const uint32_t *rle_counts,
                                  int C, const int *rle_first, const int *rle_plane, int Q, const int *sizes, int N, int H, int Wd,
                                  void *ws, uint32_t *bits, uint32_t *area_or_null, void *stream) {
    SCDA_CHECK_ARGS(sizes && bits && ws && (uintptr_t)ws % 16 == 0 && plane_ok(N, H, Wd) && V >= 0 && P >= 0 && C >= 0 && Q >= 0 &&
                    (long long)P + Q < 0x7fffffffLL, "scda_mask_frpoly_hip")
    SCDA_CHECK_ARGS(P == 0 ? V == 0 : (poly_first && poly_plane && (xy || V == 0)), "scda_mask_frpoly_hip (polygons)")
    SCDA_CHECK_ARGS(Q == 0 ? C == 0 : (rle_first && rle_plane && (rle_counts || C == 0)), "scda_mask_frpoly_hip (run lengths)")
    const size_t TW = toggle_words(H, Wd);
    const int nrb = (H + 31) / 32;
    uint32_t *tog = (uint32_t *)ws;
    hipStream_t st = as_stream(stream);
    if (P + Q > 0) {
        if (hipMemsetAsync(tog, 0, ((size_t)P + Q) * TW * sizeof(uint32_t), st) != hipSuccess) return launch_status("mask_frpoly clear");
        if (V > 0)
            hipLaunchKernelGGL(poly_toggle_kernel, dim3(cdiv(V, kThreads / kWave)), dim3(kThreads), 0, st, xy, V, poly_first, poly_plane, P,
                               sizes, N, H, Wd, TW, tog);
        if (Q > 0)
            hipLaunchKernelGGL(rle_toggle_kernel, dim3(Q), dim3(kThreads), 0, st, rle_counts, C, rle_first, rle_plane, sizes, N, H, Wd, TW,
                               tog + (size_t)P * TW);
        hipLaunchKernelGGL(parity_scan_kernel, dim3(P + Q), dim3(kThreads), 0, st, poly_plane, P, rle_plane, sizes, N, H, Wd, TW, tog);
    }
    if (area_or_null && hipMemsetAsync(area_or_null, 0, (size_t)N * sizeof(uint32_t), st) != hipSuccess)
        return launch_status("mask_frpoly clear");
    hipLaunchKernelGGL(plane_write_kernel, dim3(cdiv((long long)nrb * Wd, kThreads), N), dim3(kThreads), 0, st, poly_plane, P, rle_plane, Q,
                       sizes, N, H, Wd, nrb, TW, (const uint32_t *)tog, bits, area_or_null);
    return launch_status("mask_frpoly kernels");
}
