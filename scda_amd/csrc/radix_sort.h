// radix_sort.h -- the stable LSD radix sort of the evaluators (coco_eval.hip, map_eval.hip): 8 bits per pass over a permutation of
// row indices; per-tile histograms, one scan (block_scan256 of eval_prims.h), a stable scatter (wave match by ballots).  A pass is
// templated on the key: any struct passed by value with `__device__ uint32_t digit(uint32_t row) const`, the row's 8-bit digit of this
// pass, taken at the key's `shift`; sort_u32 runs the four passes of a 32-bit key.  The only atomics are integer LDS histogram
// counters, so a pass gives the same bytes every time.
#pragma once
#include "eval_prims.h"

namespace scda {
namespace radix {

constexpr int kSortRounds = 16, kSortTile = 64 * kSortRounds;

// float32 score -> uint32 whose ASCENDING order is the score's descending order (-0 and +0 are one key)
__device__ inline uint32_t score_descending(float s) {
    const uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

// grid (tiles), 64 threads: hist [tiles, 256]
template <class Key>
__global__ __launch_bounds__(64) void sort_hist_kernel(const uint32_t *__restrict__ src, int n, Key key, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    const int lane = threadIdx.x;
    for (int q = lane; q < 256; q += 64) h[q] = 0;
    __syncthreads();
    for (int r = 0; r < kSortRounds; ++r) {
        const int i = blockIdx.x * kSortTile + r * 64 + lane;
        if (i < n) atomicAdd(&h[key.digit(src[i])], 1u);
    }
    __syncthreads();
    for (int q = lane; q < 256; q += 64) hist[(size_t)blockIdx.x * 256 + q] = h[q];
}

// one block of 256 threads: hist [tiles, 256] -> each (tile, digit)'s first output index, digits major
static __global__ __launch_bounds__(256) void sort_scan_kernel(uint32_t *__restrict__ hist, int tiles) {
    __shared__ uint32_t wave_sums[4];
    const int d = threadIdx.x;
    uint32_t tot = 0;
    for (int b = 0; b < tiles; ++b) tot += hist[(size_t)b * 256 + d];
    uint32_t all;
    uint32_t run = block_scan256(tot, wave_sums, Add(), 0u, &all) - tot;
    for (int b = 0; b < tiles; ++b) {
        const uint32_t v = hist[(size_t)b * 256 + d];
        hist[(size_t)b * 256 + d] = run;
        run += v;
    }
}

// grid (tiles), 64 threads: 64 elements per round; a lane's place among the lanes of its digit comes from 8 ballots
template <class Key>
__global__ __launch_bounds__(64) void sort_scatter_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int n, Key key,
                                                          const uint32_t *__restrict__ offs) {
    __shared__ uint32_t base[256];
    const int lane = threadIdx.x;
    for (int q = lane; q < 256; q += 64) base[q] = offs[(size_t)blockIdx.x * 256 + q];
    __syncthreads();
    for (int r = 0; r < kSortRounds; ++r) {
        const int i = blockIdx.x * kSortTile + r * 64 + lane;
        const bool valid = i < n;
        const uint32_t e = valid ? src[i] : 0u;
        const uint32_t dg = valid ? key.digit(e) : 0u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool s = (dg >> bit) & 1u;
            const unsigned long long m = __ballot(valid && s);
            peers &= s ? m : ~m;
        }
        const int before = __popcll(peers & ((1ull << lane) - 1ull)), all = __popcll(peers);
        uint32_t pos = 0;
        if (valid) pos = base[dg] + before;
        __syncthreads();
        if (valid && before == all - 1) base[dg] += all;
        __syncthreads();
        if (valid && pos < (uint32_t)n) dst[pos] = e;
    }
}

// one stable pass: src -> dst; hist: cdiv(n, kSortTile) * 256 words
template <class Key>
inline void sort_pass(const uint32_t *src, uint32_t *dst, int n, const Key &key, uint32_t *hist, hipStream_t st) {
    const int tiles = (n + kSortTile - 1) / kSortTile;
    hipLaunchKernelGGL(sort_hist_kernel<Key>, dim3(tiles), dim3(64), 0, st, src, n, key, hist);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(256), 0, st, hist, tiles);
    hipLaunchKernelGGL(sort_scatter_kernel<Key>, dim3(tiles), dim3(64), 0, st, src, dst, n, key, (const uint32_t *)hist);
}

// the four stable passes over a 32-bit key (key.shift = 0, 8, 16, 24), between perm_a and perm_b; returns the buffer that holds the
// result (an even number of passes: perm_a again, and perm_b is free for the next pass)
template <class Key>
inline uint32_t *sort_u32(uint32_t *perm_a, uint32_t *perm_b, int n, Key key, uint32_t *hist, hipStream_t st) {
    for (int pass = 0; pass < 4; ++pass) {
        key.shift = 8 * pass;
        sort_pass(perm_a, perm_b, n, key, hist, st);
        uint32_t *t = perm_a; perm_a = perm_b; perm_b = t;
    }
    return perm_a;
}

}  // namespace radix
}  // namespace scda
