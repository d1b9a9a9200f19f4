// mask_rle.hip -- COCO run-length results from bit-packed instance masks on the device (gfx950): the per-mask primitives of
// datasets/pycocotools/common/maskApi.c (rleEncode, rleToString, rleArea, rleToBbox, rleIou) on scda_mask_paste_hip's packed planes.
// The rules are stated in include/scda_ops.h and restated in numpy by tests/mask_rle_np.py; everything here is integer arithmetic plus
// one IEEE double division, so the results are the reference's bit for bit and do not depend on any arrival order (no atomics).
//
// A thread owns a block of 32 rows x 32 columns (one packed word per row): it loads the 32 words -- neighbouring lanes read
// neighbouring words of a row --, transposes the 32 x 32 bits in registers and then holds every column of the block as one word whose
// bit i is row y0 + i.  Transitions along a column are popcount(m ^ ((m << 1) | carry)), carry = the pixel before the block's first row
// in column-major order (the row above, or the last row of the previous column).
//
//   rle_count_kernel   per block: transitions per column (uint16), set pixels, run end points' min / max          [reads the bits once]
//   rle_scan_kernel    per mask : sums the partials, turns the per-block counts into every column's first run index
//   rle_emit_kernel    per block: transition positions into the workspace at their run index                      [reads the bits again]
//   rle_string_kernel  per mask : counts = differences of positions, the 6-bit string (length, scan, bytes)
//   mask_iou_kernel    per pair : popcount(dt & gt) over the common columns, the box gate, the double division
#include "eval_prims.h"

namespace {
using namespace scda;

constexpr int kThreads = 256;                   // block_scan256 (eval_prims.h) is written for it
constexpr int kPart = 8;                        // uint32 per block partial: area, xs, xe, ys, ye (+ 3 unused: two 16-byte stores)

// the image size of mask r and the word columns [wa, wb) that have to be scanned
struct Geo { int h, w, wa, wb; };

struct Sizes {
    const float *info;                          // [*, info_stride] (h, w, ...) per image, or null: (h_all, w_all) for every mask
    int info_stride, per_image, h_all, w_all;
    const float *rois;                          // [R, roi_stride] (b, x1, y1, x2, y2): the paste's windows as a hint, or null
    int roi_stride;
};

__device__ inline int clampi(float v, int hi) { return v >= 1.0f ? (v < (float)hi ? (int)v : hi) : 1; }

// float32 -> int as scda_mask_paste_hip truncates a RoI coordinate
__device__ inline bool trunc_ok(float v, int *out) {
    if (!(v > -5.0e8f && v < 5.0e8f)) return false;
    *out = (int)v;
    return true;
}

__device__ inline Geo mask_geo(const Sizes &s, int r, int H, int Wd) {
    Geo g;
    if (s.info) {
        const float *row = s.info + (size_t)(r / s.per_image) * s.info_stride;
        g.h = clampi(row[0], H);
        g.w = clampi(row[1], Wd * 32);
    } else {
        g.h = s.h_all; g.w = s.w_all;
    }
    int ca = 0, cb = g.w;
    if (s.rois) {
        // the paste's window: a pasted mask is zero outside columns [max(x1, 0), min(x1 + roi_w, W)); the transition that closes a run
        // reaching the window's last row belongs to the column behind it, hence cb + 1
        const float *roi = s.rois + (size_t)r * s.roi_stride;
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        bool live = trunc_ok(roi[1], &x1);
        live = trunc_ok(roi[2], &y1) && live;
        live = trunc_ok(roi[3], &x2) && live;
        live = trunc_ok(roi[4], &y2) && live;
        live = live && x2 - x1 + 1 > 0 && y2 - y1 + 1 > 0;
        if (live) {
            ca = x1 > 0 ? x1 : 0;
            cb = min(x2 + 1, g.w);
            cb = min(cb + 1, g.w);
        }
        if (!live || ca >= cb) ca = cb = 0;
    }
    g.wa = ca >> 5;
    g.wb = (cb + 31) >> 5;
    return g;
}

// the block (rows y0.., word column wc) of one plane cropped to (h, w): col[j] bit i = pixel (y0 + i, 32 wc + j); carry bit j = the pixel
// before (y0, 32 wc + j) in column-major order; rowmask = the block's rows inside the crop
__device__ inline void load_block(const uint32_t *__restrict__ plane, int Wd, int h, int w, int wc, int y0, uint32_t col[32],
                                  uint32_t *carry, uint32_t *rowmask) {
    const int nr = min(32, h - y0), nc = min(32, w - 32 * wc);
    const uint32_t colmask = nc >= 32 ? 0xffffffffu : (1u << nc) - 1u;
    *rowmask = nr >= 32 ? 0xffffffffu : (1u << nr) - 1u;
    const uint32_t *p = plane + (size_t)y0 * Wd + wc;
#pragma unroll
    for (int i = 0; i < 32; ++i) col[i] = i < nr ? p[(size_t)i * Wd] & colmask : 0u;
    if (y0 > 0) {
        *carry = plane[(size_t)(y0 - 1) * Wd + wc] & colmask;
    } else {
        const uint32_t *last = plane + (size_t)(h - 1) * Wd + wc;
        const uint32_t before = wc > 0 ? last[-1] >> 31 : 0u;
        *carry = ((last[0] << 1) | before) & colmask;
    }
    transpose32(col);
}

__device__ inline bool block_of(int idx, int nrb, int Wd, const Geo &g, int *rb, int *wc) {
    if (idx >= nrb * Wd) return false;
    *rb = idx / Wd;
    *wc = idx - *rb * Wd;
    return *wc >= g.wa && *wc < g.wb && *rb * 32 < g.h;
}

// grid (ceil(nrb * Wd / 256), R).  cnt16 [R, nrb, Wd * 32] (null: the partials only), part [R, nrb, Wd, kPart]
__global__ __launch_bounds__(kThreads) void rle_count_kernel(const uint32_t *__restrict__ bits, int H, int Wd, int nrb, Sizes sz,
                                                             uint16_t *__restrict__ cnt16, uint32_t *__restrict__ part) {
    const int r = blockIdx.y;
    const Geo g = mask_geo(sz, r, H, Wd);
    int rb, wc;
    if (!block_of(blockIdx.x * kThreads + threadIdx.x, nrb, Wd, g, &rb, &wc)) return;
    const int y0 = rb * 32;
    uint32_t col[32], carry, rowmask;
    load_block(bits + (size_t)r * H * Wd, Wd, g.h, g.w, wc, y0, col, &carry, &rowmask);
    uint32_t area = 0, xs = 0xffffffffu, xe = 0, ys = 0xffffffffu, ye = 0;
    uint32_t packed[16];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const uint32_t m = col[j], c = 32 * wc + j;
        const uint32_t tr = (m ^ ((m << 1) | ((carry >> j) & 1u))) & rowmask;
        const uint32_t n = __popc(tr);
        if (j & 1) packed[j >> 1] |= n << 16; else packed[j >> 1] = n;
        area += __popc(m);
        // rleToBbox's end points: a 0 -> 1 transition is a run's first pixel, a 1 -> 0 transition follows a run's last pixel
        const uint32_t s = tr & m;
        uint32_t e = tr & ~m;
        if (y0 == 0 && (e & 1u)) {              // the run ended in the last row of the column before
            e &= ~1u;
            xs = min(xs, c - 1); xe = max(xe, c - 1);
            ys = min(ys, (uint32_t)g.h - 1); ye = max(ye, (uint32_t)g.h - 1);
        }
        if (s) {
            xs = min(xs, c); xe = max(xe, c);
            ys = min(ys, (uint32_t)(y0 + __ffs(s) - 1)); ye = max(ye, (uint32_t)(y0 + 31 - __clz(s)));
        }
        if (e) {
            xs = min(xs, c); xe = max(xe, c);
            ys = min(ys, (uint32_t)(y0 + __ffs(e) - 2)); ye = max(ye, (uint32_t)(y0 + 30 - __clz(e)));
        }
        // a mask whose very last pixel is set: its last run ends there
        if ((int)c == g.w - 1 && g.h - 1 - y0 < 32 && ((m >> ((g.h - 1 - y0) & 31)) & 1u)) {
            xs = min(xs, c); xe = max(xe, c);
            ys = min(ys, (uint32_t)g.h - 1); ye = max(ye, (uint32_t)g.h - 1);
        }
    }
    const size_t blk = ((size_t)r * nrb + rb) * Wd + wc;
    if (cnt16) {
        uint4 *dst = (uint4 *)(cnt16 + blk * 32);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = make_uint4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]);
    }
    uint4 *pp = (uint4 *)(part + blk * kPart);
    pp[0] = make_uint4(area, xs, xe, ys);
    pp[1] = make_uint4(ye, 0u, 0u, 0u);
}

// grid (R), 256 threads.  With cnt16: in place, cnt16[r, rb, c] becomes the number of transitions of column c above block rb, colbase
// [R, Wd * 32] every column's first transition index, n_runs = transitions + 1.  Always: area, bbox from the partials.
__global__ __launch_bounds__(kThreads) void rle_scan_kernel(int H, int Wd, int nrb, Sizes sz, uint16_t *__restrict__ cnt16,
                                                            const uint32_t *__restrict__ part, uint32_t *__restrict__ colbase,
                                                            int *__restrict__ n_runs, uint32_t *__restrict__ area_out,
                                                            uint32_t *__restrict__ bbox_out) {
    __shared__ uint32_t wave_sums[kThreads / 64];
    __shared__ uint32_t red[5][kThreads / 64];
    const int r = blockIdx.x, t = threadIdx.x;
    const Geo g = mask_geo(sz, r, H, Wd);
    const int nrbv = (g.h + 31) >> 5, nw = g.wb - g.wa;
    // ---- the partials
    uint32_t area = 0, xs = 0xffffffffu, xe = 0, ys = 0xffffffffu, ye = 0;
    for (int i = t; i < nrbv * nw; i += kThreads) {
        const int rb = i / nw, wc = g.wa + i - rb * nw;
        const uint4 *pp = (const uint4 *)(part + (((size_t)r * nrb + rb) * Wd + wc) * kPart);
        const uint4 a = pp[0];
        area += a.x; xs = min(xs, a.y); xe = max(xe, a.z); ys = min(ys, a.w); ye = max(ye, pp[1].x);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        area += __shfl_xor(area, d, 64);
        xs = min(xs, __shfl_xor(xs, d, 64)); xe = max(xe, __shfl_xor(xe, d, 64));
        ys = min(ys, __shfl_xor(ys, d, 64)); ye = max(ye, __shfl_xor(ye, d, 64));
    }
    if ((t & 63) == 0) {
        red[0][t >> 6] = area; red[1][t >> 6] = xs; red[2][t >> 6] = xe; red[3][t >> 6] = ys; red[4][t >> 6] = ye;
    }
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < kThreads / 64; ++q) {
            area += red[0][q]; xs = min(xs, red[1][q]); xe = max(xe, red[2][q]); ys = min(ys, red[3][q]); ye = max(ye, red[4][q]);
        }
        area_out[r] = area;
        uint32_t *bb = bbox_out + (size_t)r * 4;
        if (area == 0) {
            bb[0] = bb[1] = bb[2] = bb[3] = 0;
        } else {
            bb[0] = xs; bb[1] = ys; bb[2] = xe - xs + 1; bb[3] = ye - ys + 1;
        }
    }
    if (!cnt16) return;
    // ---- every column's first transition index
    uint32_t base = 0;
    for (int c0 = 32 * g.wa; c0 < 32 * g.wb; c0 += kThreads) {
        const int c = c0 + t;
        uint32_t tot = 0;
        if (c < 32 * g.wb) {
            uint16_t *p = cnt16 + (size_t)r * nrb * Wd * 32 + c;
            for (int rb = 0; rb < nrbv; ++rb, p += (size_t)Wd * 32) {
                const uint32_t v = *p;
                *p = (uint16_t)tot;
                tot += v;
            }
        }
        uint32_t total;
        const uint32_t ex = block_scan256(tot, wave_sums, Add(), base, &total) - tot;
        if (c < 32 * g.wb) colbase[(size_t)r * Wd * 32 + c] = base + ex;
        base = total;
    }
    if (t == 0) n_runs[r] = (int)base + 1;
}

// grid as rle_count_kernel.  pos [R, cap_runs]: the column-major position of transition k, k < cap_runs
__global__ __launch_bounds__(kThreads) void rle_emit_kernel(const uint32_t *__restrict__ bits, int H, int Wd, int nrb, Sizes sz,
                                                            const uint16_t *__restrict__ cnt16, const uint32_t *__restrict__ colbase,
                                                            int cap_runs, uint32_t *__restrict__ pos) {
    const int r = blockIdx.y;
    const Geo g = mask_geo(sz, r, H, Wd);
    int rb, wc;
    if (!block_of(blockIdx.x * kThreads + threadIdx.x, nrb, Wd, g, &rb, &wc)) return;
    const int y0 = rb * 32;
    uint32_t col[32], carry, rowmask;
    load_block(bits + (size_t)r * H * Wd, Wd, g.h, g.w, wc, y0, col, &carry, &rowmask);
    const size_t blk = ((size_t)r * nrb + rb) * Wd + wc;
    uint32_t above[16], first[32];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = ((const uint4 *)(cnt16 + blk * 32))[q];
        above[4 * q] = v.x; above[4 * q + 1] = v.y; above[4 * q + 2] = v.z; above[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 v = ((const uint4 *)(colbase + (size_t)r * Wd * 32 + 32 * wc))[q];
        first[4 * q] = v.x; first[4 * q + 1] = v.y; first[4 * q + 2] = v.z; first[4 * q + 3] = v.w;
    }
    uint32_t *out = pos + (size_t)r * cap_runs;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const uint32_t m = col[j];
        uint32_t tr = (m ^ ((m << 1) | ((carry >> j) & 1u))) & rowmask;
        uint32_t k = first[j] + ((j & 1) ? above[j >> 1] >> 16 : above[j >> 1] & 0xffffu);
        const uint32_t p0 = (uint32_t)(32 * wc + j) * (uint32_t)g.h + (uint32_t)y0;
        while (tr) {
            const int i = __ffs(tr) - 1;
            tr &= tr - 1;
            if (k < (uint32_t)cap_runs) out[k] = p0 + i;
            ++k;
        }
    }
}

// rleToString's characters of one count difference; returns their number and, with dst, writes them
__device__ inline int rle_chars(long long x, unsigned char *dst) {
    int n = 0;
    bool more = true;
    while (more) {
        int c = (int)(x & 0x1f);
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        if (more) c |= 0x20;
        if (dst) dst[n] = (unsigned char)(c + 48);
        ++n;
    }
    return n;
}

// grid (R), 256 threads
__global__ __launch_bounds__(kThreads) void rle_string_kernel(int H, int Wd, Sizes sz, const uint32_t *__restrict__ pos, int cap_runs,
                                                              int cap_bytes, const int *__restrict__ n_runs,
                                                              uint32_t *__restrict__ counts, int *__restrict__ n_bytes,
                                                              unsigned char *__restrict__ chars) {
    __shared__ uint32_t wave_sums[kThreads / 64];
    const int r = blockIdx.x, t = threadIdx.x;
    const int n = n_runs[r];
    if (n > cap_runs) {                                                 // overflow: n_runs says so, nothing else of this mask is usable
        if (t == 0) n_bytes[r] = 0;
        return;
    }
    const Geo g = mask_geo(sz, r, H, Wd);
    const uint32_t a = (uint32_t)g.h * (uint32_t)g.w;
    const uint32_t *p = pos + (size_t)r * cap_runs;
    uint32_t base = 0;
    for (int k0 = 0; k0 < n; k0 += kThreads) {
        const int k = k0 + t;
        long long x = 0;
        int len = 0;
        if (k < n) {
            // run k lies between transition k - 1 (or the start) and transition k (or the end)
            const uint32_t e1 = k < n - 1 ? p[k] : a, e0 = k > 0 ? p[k - 1] : 0u;
            const uint32_t cnt = e1 - e0;
            counts[(size_t)r * cap_runs + k] = cnt;
            x = (long long)cnt;
            if (k > 2) x -= (long long)(p[k - 2] - (k > 2 ? p[k - 3] : 0u));
            len = rle_chars(x, nullptr);
        }
        uint32_t total;
        const uint32_t off = base + block_scan256((uint32_t)len, wave_sums, Add(), base, &total) - (uint32_t)len;
        if (k < n && off + (uint32_t)len <= (uint32_t)cap_bytes) rle_chars(x, chars + (size_t)r * cap_bytes + off);
        base = total;
    }
    if (t == 0) n_bytes[r] = (int)base;
}

// grid (M, N), 256 threads.  stats: area [M + N] and bbox [M + N, 4] of dt then gt
__global__ __launch_bounds__(kThreads) void mask_iou_kernel(const uint32_t *__restrict__ dt, const uint32_t *__restrict__ gt, int M, int H,
                                                            int Wd, int h, int w, const unsigned char *__restrict__ iscrowd,
                                                            const uint32_t *__restrict__ area, const uint32_t *__restrict__ bbox,
                                                            double *__restrict__ iou, uint32_t *__restrict__ inter) {
    __shared__ uint32_t red[kThreads / 64];
    const int d = blockIdx.x, gi = blockIdx.y, t = threadIdx.x;
    const uint32_t *db = bbox + (size_t)d * 4, *gb = bbox + (size_t)(M + gi) * 4;
    const uint32_t da = area[d], ga = area[M + gi];
    uint32_t n = 0;
    if (da && ga) {
        // the boxes' column ranges are exact (every run's first and last pixel enter them); their rows are not (see rleToBbox)
        const int xa = max(db[0], gb[0]), xb = min(db[0] + db[2], gb[0] + gb[2]);      // [xa, xb)
        if (xa < xb) {
            const int w0 = xa >> 5, nw = ((xb + 31) >> 5) - w0, wl = (w - 1) >> 5;
            const uint32_t lastmask = (w & 31) ? (1u << (w & 31)) - 1u : 0xffffffffu;
            const uint32_t *pd = dt + (size_t)d * H * Wd, *pg = gt + (size_t)gi * H * Wd;
            for (int i = t; i < h * nw; i += kThreads) {
                const int y = i / nw, wc = w0 + i - y * nw;
                uint32_t v = pd[(size_t)y * Wd + wc] & pg[(size_t)y * Wd + wc];
                if (wc == wl) v &= lastmask;
                n += __popc(v);
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s, 64);
    if ((t & 63) == 0) red[t >> 6] = n;
    __syncthreads();
    if (t != 0) return;
    for (int q = 1; q < kThreads / 64; ++q) n += red[q];
    // bbIou's gate on the two rleToBbox boxes, then rleIou's ratio
    const long long bw = min((long long)db[2] + db[0], (long long)gb[2] + gb[0]) - max((long long)db[0], (long long)gb[0]);
    const long long bh = min((long long)db[3] + db[1], (long long)gb[3] + gb[1]) - max((long long)db[1], (long long)gb[1]);
    double o = 0.0;
    if (bw > 0 && bh > 0 && n > 0) {
        const uint32_t u = (iscrowd && iscrowd[gi]) ? da : da + ga - n;
        o = (double)n / (double)u;
    }
    iou[(size_t)gi * M + d] = o;
    inter[(size_t)gi * M + d] = n;
}

struct Layout { size_t cnt16, part, colbase, pos, total; int nrb; };

Layout layout(int R, int H, int Wd, int cap_runs) {
    Layout l;
    l.nrb = (H + 31) / 32;
    const size_t blocks = (size_t)R * l.nrb * Wd;
    Bump ws;
    l.cnt16 = ws.take(blocks * 32 * sizeof(uint16_t));
    l.part = ws.take(blocks * kPart * sizeof(uint32_t));
    l.colbase = ws.take((size_t)R * Wd * 32 * sizeof(uint32_t));
    l.pos = ws.take((size_t)R * (cap_runs > 0 ? cap_runs : 0) * sizeof(uint32_t));
    l.total = ws.total();
    return l;
}

// scda_mask_iou_hip's workspace: the partials of the M + N planes, then area [M + N] and bbox [M + N, 4]
struct IouLayout { size_t part, area, total; int nrb; };

IouLayout iou_layout(int planes, int H, int Wd) {
    IouLayout l;
    l.nrb = (H + 31) / 32;
    Bump ws;
    l.part = ws.take((size_t)planes * l.nrb * Wd * kPart * sizeof(uint32_t));
    l.area = ws.take((size_t)planes * 5 * sizeof(uint32_t));
    l.total = ws.total();
    return l;
}

int bitlength(unsigned long long v) {
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

bool plane_ok(int R, int H, int Wd) {
    return R > 0 && R <= 65535 && H > 0 && H <= 65535 && Wd > 0 && Wd <= 2047 && (long long)H * Wd * 32 < 0x7fffffffLL;
}

}  // namespace

SCDA_API int scda_mask_rle_max_chars(int h, int w) {
    if (h <= 0 || w <= 0) return 0;
    return (bitlength((unsigned long long)h * (unsigned long long)w) + 1 + 4) / 5;
}

SCDA_API size_t scda_mask_rle_workspace_bytes(int R, int H, int Wd, int cap_runs) {
    if (!plane_ok(R, H, Wd) || cap_runs < 0) return 0;
    return layout(R, H, Wd, cap_runs).total;
}

SCDA_API int scda_mask_rle_hip(const uint32_t *bits, int R, int H, int Wd, const float *image_info, int info_stride, int masks_per_image,
                               int h_all, int w_all, const float *rois_or_null, int roi_stride, int cap_runs, int cap_bytes, void *ws,
                               int *n_runs, uint32_t *counts, int *n_bytes, unsigned char *chars, uint32_t *area, uint32_t *bbox,
                               void *stream) {
    SCDA_CHECK_ARGS(bits && ws && n_runs && counts && n_bytes && chars && area && bbox && plane_ok(R, H, Wd) && cap_runs >= 1 &&
                    (uintptr_t)ws % 16 == 0, "scda_mask_rle_hip")
    SCDA_CHECK_ARGS(image_info ? (info_stride >= 2 && masks_per_image >= 1) : (h_all >= 1 && h_all <= H && w_all >= 1 && w_all <= Wd * 32),
                    "scda_mask_rle_hip (sizes)")
    SCDA_CHECK_ARGS(!rois_or_null || roi_stride >= 5, "scda_mask_rle_hip (rois)")
    SCDA_CHECK_ARGS((long long)cap_bytes >= (long long)cap_runs * scda_mask_rle_max_chars(H, Wd * 32) &&
                    (long long)cap_runs * R < 0x7fffffffLL, "scda_mask_rle_hip (cap_bytes < cap_runs * scda_mask_rle_max_chars(H, 32 Wd))")
    const Layout l = layout(R, H, Wd, cap_runs);
    char *w8 = (char *)ws;
    uint16_t *cnt16 = (uint16_t *)(w8 + l.cnt16);
    uint32_t *part = (uint32_t *)(w8 + l.part), *colbase = (uint32_t *)(w8 + l.colbase), *pos = (uint32_t *)(w8 + l.pos);
    const Sizes sz = {image_info, info_stride, masks_per_image, h_all, w_all, rois_or_null, roi_stride};
    const dim3 grid(cdiv((long long)l.nrb * Wd, kThreads), R);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rle_count_kernel, grid, dim3(kThreads), 0, st, bits, H, Wd, l.nrb, sz, cnt16, part);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(R), dim3(kThreads), 0, st, H, Wd, l.nrb, sz, cnt16, (const uint32_t *)part, colbase, n_runs,
                       area, bbox);
    hipLaunchKernelGGL(rle_emit_kernel, grid, dim3(kThreads), 0, st, bits, H, Wd, l.nrb, sz, (const uint16_t *)cnt16,
                       (const uint32_t *)colbase, cap_runs, pos);
    hipLaunchKernelGGL(rle_string_kernel, dim3(R), dim3(kThreads), 0, st, H, Wd, sz, (const uint32_t *)pos, cap_runs, cap_bytes,
                       (const int *)n_runs, counts, n_bytes, chars);
    return launch_status("mask_rle kernels");
}

SCDA_API size_t scda_mask_iou_workspace_bytes(int M, int N, int H, int Wd) {
    if (M <= 0 || N <= 0 || !plane_ok(M + N, H, Wd)) return 0;
    return iou_layout(M + N, H, Wd).total;
}

SCDA_API int scda_mask_iou_hip(const uint32_t *dt_bits, int M, const uint32_t *gt_bits, int N, int H, int Wd, int h, int w,
                               const unsigned char *iscrowd_or_null, void *ws, double *iou, uint32_t *inter, void *stream) {
    SCDA_CHECK_ARGS(dt_bits && gt_bits && ws && iou && inter && M > 0 && N > 0 && M <= 65535 && N <= 65535 && plane_ok(M + N, H, Wd) &&
                    h >= 1 && h <= H && w >= 1 && w <= Wd * 32 && (uintptr_t)ws % 16 == 0, "scda_mask_iou_hip")
    const IouLayout l = iou_layout(M + N, H, Wd);
    const int nrb = l.nrb;
    uint32_t *part = (uint32_t *)((char *)ws + l.part), *area = (uint32_t *)((char *)ws + l.area);
    uint32_t *bbox = area + (M + N);
    const Sizes sz = {nullptr, 0, 1, h, w, nullptr, 0};
    hipStream_t st = as_stream(stream);
    const size_t per = (size_t)nrb * Wd * kPart;
    hipLaunchKernelGGL(rle_count_kernel, dim3(cdiv((long long)nrb * Wd, kThreads), M), dim3(kThreads), 0, st, dt_bits, H, Wd, nrb, sz,
                       (uint16_t *)nullptr, part);
    hipLaunchKernelGGL(rle_count_kernel, dim3(cdiv((long long)nrb * Wd, kThreads), N), dim3(kThreads), 0, st, gt_bits, H, Wd, nrb, sz,
                       (uint16_t *)nullptr, part + per * M);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(M + N), dim3(kThreads), 0, st, H, Wd, nrb, sz, (uint16_t *)nullptr, (const uint32_t *)part,
                       (uint32_t *)nullptr, (int *)nullptr, area, bbox);
    hipLaunchKernelGGL(mask_iou_kernel, dim3(M, N), dim3(kThreads), 0, st, dt_bits, gt_bits, M, H, Wd, h, w, iscrowd_or_null,
                       (const uint32_t *)area, (const uint32_t *)bbox, iou, inter);
    return launch_status("mask_iou kernels");
}
