// eval_prims.h -- what the device evaluators and result kernels share (coco_eval.hip, map_eval.hip, mask_rle.hip, mask_poly.hip and,
// through radix_sort.h, the sort): the 256-thread block scan, the reversed precision envelope, the stable wave compaction, the segment
// bounds of sorted rows; on the host the workspace bump allocator and the argument check of the C-ABI entries.  Each exists once, here.
#pragma once
#include "common.h"

// the argument check of a C-ABI entry point
#define SCDA_CHECK_ARGS(cond, name) if (!(cond)) { set_error(name ": bad arguments"); return SCDA_EINVAL; }

namespace scda {

// ---------------------------------------------------------------------------------------------------------------- host
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace layout: consecutive 256-byte aligned pieces
struct Bump {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += align256(bytes); return o; }
    size_t total() const { return at; }
};

// -------------------------------------------------------------------------------------------------------------- device
struct Add { template <class T> __device__ T operator()(const T &a, const T &b) const { return a + b; } };
struct FMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// the value of lane - d; a struct scanned as one value overloads this member-wise next to its definition
template <class T> __device__ inline T lanes_up(T v, int d) { return __shfl_up(v, d, 64); }

// Scan of one value per thread over a block of 256 threads (4 waves) in thread order: returns op over the values of threads 0 .. this
// one (the exclusive sum is that minus v); *total = op(carry, every thread's value), the carry of the next round.  wave_part: 4 values
// in LDS.  Two barriers: the previous use of wave_part is over; the partials are written.
template <class T, class Op>
__device__ inline T block_scan256(T v, T *wave_part, Op op, T carry, T *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = lanes_up(inc, d);
        if (lane >= d) inc = op(inc, o);
    }
    __syncthreads();
    if (lane == 63) wave_part[wv] = inc;
    __syncthreads();
    T all = carry;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < wv) inc = op(inc, wave_part[q]);
        all = op(all, wave_part[q]);
    }
    *total = all;
    return inc;
}

// One 256-row round of a precision envelope whose rows are visited from the LAST to the first: pm = the row's precision (-1: no row)
// -> the maximum over the row and everything behind it; *c_max carries the maximum of the rounds done (-1 before the first)
__device__ inline double envelope_step(double pm, double *w_max, double *c_max) {
    double all;
    pm = fmax(block_scan256(pm, w_max, FMax(), *c_max, &all), *c_max);
    *c_max = all;
    return pm;
}

// stable compaction by one wave: val(i) of the indices i < n with pred(i), in order, appended to list at cnt (wave-uniform); -> the new cnt
template <class Pred, class Val>
__device__ inline int wave_compact(int n, int lane, uint16_t *list, int cnt, Pred pred, Val val) {
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool f = i < n && pred(i);
        const unsigned long long m = __ballot(f);
        if (f) list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)val(i);
        cnt += __popcll(m);
    }
    return cnt;
}

template <class Pred>
__device__ inline int wave_compact(int n, int lane, uint16_t *list, int cnt, Pred pred) {
    return wave_compact(n, lane, list, cnt, pred, [](int i) { return i; });
}

// grid (cdiv(n, 256)), 256 threads.  seg [2, stride] (zeroed before): the first row and the END of the segment of every value key(i)
// takes over the n sorted rows
template <class Key>
__global__ __launch_bounds__(256) void segment_bounds_kernel(int n, Key key, int stride, int *__restrict__ seg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = key(i);
    if (i == 0 || key(i - 1) != c) seg[c] = i;
    if (i == n - 1 || key(i + 1) != c) seg[stride + c] = i + 1;
}

}  // namespace scda
