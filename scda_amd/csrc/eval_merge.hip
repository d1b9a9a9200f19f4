// eval_merge.hip -- merging sharded device evaluators (gfx950): the rows that data-parallel ranks collected, gathered shard by shard,
// are placed into one evaluator's row arrays in a given shard order, the counters are summed, and images that occur more than once
// (a sampler's padding) are marked.  The rules M1..M4 are stated in include/scda_ops.h and restated in numpy by
// tests/sharded_map_np.py.  Everything is integer work: copies, one stable sort, two block scans; the only atomics are the sort's LDS
// histogram counters, so two runs give the same bytes.
//
//   place_rows_kernel        per destination image: its shard and row from the prefix sums of the counts, copy or fill          (M1)
//   sum_counters_kernel      dst[j] += the shards' counters                                                                     (M2)
//   iota_kernel, radix_sort.h by image id; mark_duplicates_kernel: one block, the run heads by block_scan256 (maximum)          (M3)
//   map_duplicates_kernel    per later copy: compare the rows with the first copy's, zero tp                                    (M4)
// The block scan and the workspace allocator are those of eval_prims.h, the sort is radix_sort.h's.
#include "eval_prims.h"
#include "radix_sort.h"

namespace {
using namespace scda;

constexpr int kMaxShards = 256, kMaxPer = 1024;

struct IMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };

struct PlaceArgs {
    const uint32_t *src;                        // [W, cap, row_words]
    uint32_t *dst;                              // [max_images, row_words]
    const int *counts_dev;                      // [W] or null: then counts[] holds them
    int *flags;
    int W, cap, row_words, start, max_images, fill;
    int order[kMaxShards], counts[kMaxShards];
};

// grid (images to write), 256 threads: destination image start + blockIdx.x
__global__ __launch_bounds__(256) void place_rows_kernel(PlaceArgs p) {
    const int j = blockIdx.x, tid = threadIdx.x;
    const int room = p.max_images - p.start;
    // the shard and the row of the j-th merged image: a walk over the counts in shard order (block-uniform)
    int shard = -1, row = 0;
    long long before = 0;
    for (int k = 0; k < p.W; ++k) {
        const int s = p.order[k];
        int c = p.counts_dev ? p.counts_dev[s] : p.counts[s];
        c = min(max(c, 0), p.cap);
        if (shard < 0 && (long long)j < before + c) { shard = s; row = (int)((long long)j - before); }
        before += c;
    }
    if (j == 0 && tid == 0 && p.counts_dev) {
        if (before > (long long)room) p.flags[0] = 1;
        p.flags[3] = p.start + (int)(before < (long long)room ? before : (long long)room);
    }
    if (j >= room) return;
    uint32_t *out = p.dst + (size_t)(p.start + j) * p.row_words;
    if (shard >= 0) {
        const uint32_t *in = p.src + ((size_t)shard * p.cap + row) * p.row_words;
        for (int w = tid; w < p.row_words; w += 256) out[w] = in[w];
    } else {
        for (int w = tid; w < p.row_words; w += 256) out[w] = p.fill == 1 ? (uint32_t)w : p.fill == 2 ? 0xffffffffu : 0u;
    }
}

__global__ __launch_bounds__(256) void sum_counters_kernel(const int *__restrict__ src, int W, int n, int *__restrict__ dst) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    int s = dst[j];
    for (int w = 0; w < W; ++w) s += src[(size_t)w * n + j];
    dst[j] = s;
}

__global__ __launch_bounds__(256) void iota_kernel(uint32_t *__restrict__ perm, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (uint32_t)i;
}

// ascending signed image id; the sort is stable, so the positions of one id stay ascending
struct IdKey {
    int shift;
    const int *ids;
    __device__ uint32_t digit(uint32_t e) const { return ((((uint32_t)ids[e]) ^ 0x80000000u) >> shift) & 255u; }
};

// one block of 256 threads over the n sorted positions, 256 a round.  A position is a duplicate when its predecessor holds the same
// id >= 0; the head of its run is the maximum over the positions so far of (head ? position : -1)
__global__ __launch_bounds__(256) void mark_duplicates_kernel(const uint32_t *__restrict__ perm, const int *__restrict__ ids, int n,
                                                              int *__restrict__ first, int *__restrict__ flags, int raise) {
    __shared__ int w_head[4];
    __shared__ uint32_t w_cnt[4];
    const int tid = threadIdx.x;
    int c_head = -1;
    uint32_t c_cnt = 0;
    for (int base = 0; base < n; base += 256) {
        const int j = base + tid;
        bool dup = false;
        uint32_t e = 0;
        if (j < n) {
            e = perm[j];
            const int id = ids[e];
            dup = j > 0 && id >= 0 && ids[perm[j - 1]] == id;
        }
        int all_head;
        const int inc = block_scan256((j < n && !dup) ? j : -1, w_head, IMax(), c_head, &all_head);
        const int head = inc > c_head ? inc : c_head;
        uint32_t all_cnt;
        block_scan256(dup ? 1u : 0u, w_cnt, Add(), c_cnt, &all_cnt);
        if (j < n) first[e] = (dup && head >= 0) ? (int)perm[head] : -1;
        c_head = all_head;
        c_cnt = all_cnt;
    }
    if (tid == 0) {
        flags[2] = (int)c_cnt;
        if (raise && c_cnt) flags[1] = 1;
    }
}

struct MapDupArgs {
    const int *first, *box, *cls, *rank, *kept;
    const float *score;
    int *tp, *flags;
    int n, D;
};

// grid (n), 256 threads: image blockIdx.x, if it is a later copy
__global__ __launch_bounds__(256) void map_duplicates_kernel(MapDupArgs p) {
    const int i = blockIdx.x;
    const int f = p.first[i];
    if (f < 0 || f >= p.n || f == i) return;
    bool differs = false;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        const size_t a = (size_t)i * p.D + d, b = (size_t)f * p.D + d;
        differs |= __float_as_uint(p.score[a]) != __float_as_uint(p.score[b]) || p.cls[a] != p.cls[b] || p.rank[a] != p.rank[b] ||
                   p.kept[a] != p.kept[b];
        for (int q = 0; q < 4; ++q) differs |= p.box[a * 4 + q] != p.box[b * 4 + q];
        p.tp[a] = 0;
    }
    if (differs) p.flags[1] = 1;
}

struct DupLayout { size_t perm_a, perm_b, hist, total; };

DupLayout dup_layout(int n) {
    DupLayout l;
    const size_t tiles = ((size_t)n + radix::kSortTile - 1) / radix::kSortTile;
    Bump ws;
    l.perm_a = ws.take((size_t)n * 4); l.perm_b = ws.take((size_t)n * 4);
    l.hist = ws.take(tiles * 256 * 4);
    l.total = ws.total();
    return l;
}

}  // namespace

SCDA_API int scda_eval_place_rows_hip(const void *src, int W, int cap, int row_words, const int *order_host, const int *counts_host_or_null,
                                      const int *counts_dev_or_null, int start, int max_images, int fill, void *dst, int *flags,
                                      void *stream) {
    SCDA_CHECK_ARGS(src && order_host && dst && flags && (counts_host_or_null != nullptr) != (counts_dev_or_null != nullptr) &&
                    (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0, "scda_eval_place_rows_hip")
    SCDA_CHECK_ARGS(W > 0 && W <= kMaxShards && cap > 0 && row_words > 0 && start >= 0 && max_images > 0 && start <= max_images &&
                    fill >= 0 && fill <= 2 && (long long)W * cap * row_words < 0x7fffffffLL &&
                    (long long)max_images * row_words < 0x7fffffffLL, "scda_eval_place_rows_hip (limits: at most 256 shards)")
    PlaceArgs args = {(const uint32_t *)src, (uint32_t *)dst, counts_dev_or_null, flags, W, cap, row_words, start, max_images, fill, {}, {}};
    bool seen[kMaxShards] = {};
    long long total = 0;
    for (int k = 0; k < W; ++k) {
        const int s = order_host[k];
        SCDA_CHECK_ARGS(s >= 0 && s < W && !seen[s], "scda_eval_place_rows_hip (order must be a permutation of the shards)")
        seen[s] = true;
        args.order[k] = s;
        if (counts_host_or_null) {
            const int c = counts_host_or_null[s];
            SCDA_CHECK_ARGS(c >= 0 && c <= cap, "scda_eval_place_rows_hip (a shard's count exceeds its capacity)")
            args.counts[s] = c;
            total += c;
        }
    }
    int blocks;
    if (counts_host_or_null) {
        SCDA_CHECK_ARGS(start + total <= max_images, "scda_eval_place_rows_hip (the merged images exceed max_images)")
        blocks = (int)total;
    } else {
        blocks = max_images - start > 0 ? max_images - start : 1;      // every remaining slot: a row or the fill; block 0 raises the flag
    }
    if (blocks == 0) return SCDA_OK;
    hipLaunchKernelGGL(place_rows_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), args);
    return launch_status("place_rows_kernel");
}

SCDA_API int scda_eval_sum_counters_hip(const int *src, int W, int n, int *dst, void *stream) {
    SCDA_CHECK_ARGS(src && dst && W > 0 && W <= kMaxShards && n > 0 && (long long)W * n < 0x7fffffffLL, "scda_eval_sum_counters_hip")
    hipLaunchKernelGGL(sum_counters_kernel, dim3(cdiv(n, 256)), dim3(256), 0, as_stream(stream), src, W, n, dst);
    return launch_status("sum_counters_kernel");
}

SCDA_API size_t scda_eval_mark_duplicates_workspace_bytes(int n) {
    if (n <= 0 || n >= 0x7fffffff / 4) return 0;
    return dup_layout(n).total;
}

SCDA_API int scda_eval_mark_duplicates_hip(const int *image_ids, int n, void *ws, int *first, int *flags, int raise_on_duplicate,
                                           void *stream) {
    SCDA_CHECK_ARGS(image_ids && ws && first && flags && (uintptr_t)ws % 16 == 0 && n > 0 && n < 0x7fffffff / 4,
                    "scda_eval_mark_duplicates_hip")
    const DupLayout l = dup_layout(n);
    char *w8 = (char *)ws;
    uint32_t *perm_a = (uint32_t *)(w8 + l.perm_a), *perm_b = (uint32_t *)(w8 + l.perm_b), *hist = (uint32_t *)(w8 + l.hist);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(iota_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, perm_a, n);
    perm_a = radix::sort_u32(perm_a, perm_b, n, IdKey{0, image_ids}, hist, st);
    hipLaunchKernelGGL(mark_duplicates_kernel, dim3(1), dim3(256), 0, st, (const uint32_t *)perm_a, image_ids, n, first, flags,
                       raise_on_duplicate);
    return launch_status("mark duplicates kernels");
}

SCDA_API int scda_map_merge_duplicates_hip(const int *first, int n, int D, const int *box, const float *score, const int *cls,
                                           const int *rank, const int *kept, int *tp, int *flags, void *stream) {
    SCDA_CHECK_ARGS(first && box && score && cls && rank && kept && tp && flags, "scda_map_merge_duplicates_hip")
    SCDA_CHECK_ARGS(n > 0 && D > 0 && D <= kMaxPer && (long long)n * D * 4 < 0x7fffffffLL, "scda_map_merge_duplicates_hip (limit: D <= 1024)")
    const MapDupArgs args = {first, box, cls, rank, kept, score, tp, flags, n, D};
    hipLaunchKernelGGL(map_duplicates_kernel, dim3(n), dim3(256), 0, as_stream(stream), args);
    return launch_status("map_duplicates_kernel");
}
