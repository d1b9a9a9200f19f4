// detection_ops.hip -- NMS, RoIPool, RoIAlign, focal loss and box-overlap
// kernels for gfx950 (wave64), behind the C ABI of include/scda_ops.h.
//
// All of these are HBM/L2-bound integer-and-compare work; none is GEMM shaped.
// This translation unit is compiled with -ffp-contract=off: the operators are
// defined (oracle/scda_oracle.c) as one IEEE fp32 operation per source operator,
// and the NMS keep list / RoIPool argmax must be bit-identical to that.
#include <float.h>
#include <stdarg.h>

#include <mutex>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

namespace scda {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// nullptr if the allocation fails: every caller checks and returns SCDA_ELAUNCH (the gathers would dereference it)
const float *zero_page() {
    static const float *pages[64] = {nullptr};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (!pages[dev]) {
        void *p = nullptr;
        if (hipMalloc(&p, 4096) == hipSuccess && hipMemset(p, 0, 4096) == hipSuccess) pages[dev] = (const float *)p;
    }
    return pages[dev];
}

// ---- launch profiler (see common.h) ----------------------------------------
struct ProfRec { int kernel; double flops, bytes; hipEvent_t a, b; };
static unsigned g_prof_mask = 0;  // bit k set: time launches of kernel class k
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_prof_pool;
static hipEvent_t prof_event() {
    hipEvent_t e;
    if (!g_prof_pool.empty()) { e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    (void)hipEventCreate(&e);
    return e;
}
// Launches come from two host threads (the Python main thread and autograd's backward thread): the record list is guarded by a
// mutex, and "which record does this thread's prof_end() close" is per thread (a begin on one thread can no longer be closed by an
// end on the other).
static std::mutex g_prof_mu;
static thread_local long g_prof_open = -1;   // index of the record this thread opened, or -1
void prof_begin(int kernel, double flops, hipStream_t st, double bytes) {
    g_prof_open = -1;
    if (!((g_prof_mask >> kernel) & 1u)) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    ProfRec r{kernel, flops, bytes, prof_event(), prof_event()};
    (void)hipEventRecord(r.a, st);
    g_prof.push_back(r);
    g_prof_open = (long)g_prof.size() - 1;
}
void prof_end(hipStream_t st) {
    if (g_prof_open < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if ((size_t)g_prof_open < g_prof.size()) (void)hipEventRecord(g_prof[g_prof_open].b, st);
    g_prof_open = -1;
}

// ---------------------------------------------------------------------------
// NMS.  Reference: extensions/_nms/src/cuda/nms_kernel.cu:16-70 (bit mask) and
// extensions/_nms/src/nms_cuda.c:47-58 (greedy sweep, on the host there).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float iou_plus1(const float *a, const float *b) {
    float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
    float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
    float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
    float interS = width * height;
    float Sa = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
    float Sb = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    return __fdiv_rn(interS, (Sa + Sb - interS));
}

// One wave per (row block, column block) of 64x64 box pairs; a 64-wide block is
// exactly one gfx950 wavefront, so the 64 column boxes sit in LDS and every lane
// owns one row box and emits one 64-bit word.  Only col_block >= row_block is
// computed: the sweep never reads the lower triangle (nms_cuda.c:53 starts at
// j = nblock); those workgroups exit at once.
// seg (may be null): SEGMENTED form -- blockIdx.z = segment s with seg[3 s .. 3 s + 2] = {first box row, box count, first mask word}:
// independent lists in one launch (the per-class lists of functions/predict_bbox.py:29-55), block-diagonal by construction.
__global__ __launch_bounds__(64) void nms_mask_kernel(const int n_, const float thresh, const float *__restrict__ boxes,
                                                       uint64_t *__restrict__ mask, const int col_blocks_,
                                                       const long long *__restrict__ seg) {
    int n = n_, col_blocks = col_blocks_;
    if (seg) {
        const long long *d = seg + 3 * blockIdx.z;
        boxes += d[0] * 5; n = (int)d[1]; mask += d[2];
        col_blocks = (n + 63) / 64;
        if ((int)blockIdx.x >= col_blocks || (int)blockIdx.y >= col_blocks) return;
    }
    const int row_start = blockIdx.y;
    const int col_start = blockIdx.x;
    if (col_start < row_start) return;  // lower triangle is never read by the sweep
    const int row_size = min(n - row_start * 64, 64);
    const int col_size = min(n - col_start * 64, 64);

    __shared__ float bb[64 * 5];
    // 320 contiguous floats of the column block: 5 coalesced passes of 64 lanes
    const float *src = boxes + (size_t)col_start * 64 * 5;
    for (int k = threadIdx.x; k < col_size * 5; k += 64) bb[k] = src[k];
    __syncthreads();

    if ((int)threadIdx.x < row_size) {
        const int cur = row_start * 64 + threadIdx.x;
        float me[4];
        me[0] = boxes[(size_t)cur * 5 + 0];
        me[1] = boxes[(size_t)cur * 5 + 1];
        me[2] = boxes[(size_t)cur * 5 + 2];
        me[3] = boxes[(size_t)cur * 5 + 3];
        uint64_t bits = 0;
        const int start = (row_start == col_start) ? (int)threadIdx.x + 1 : 0;
        for (int i = 0; i < col_size; ++i) {  // uniform trip count: LDS reads broadcast
            float v = iou_plus1(me, bb + i * 5);
            if (i >= start && v > thresh) bits |= 1ULL << i;
        }
        mask[(size_t)cur * col_blocks + col_start] = bits;
    }
}

// Greedy sweep on the device: one 1024-thread workgroup walks the 64-box chunks, FOUR at a time.
// Per group of G = 4 chunks, wave 0 resolves the 4 x 64 in-group decisions alone -- per chunk a fixpoint iteration on the wave's
// 64 diagonal words (see there), with the group's own kept rows folded into the later chunks of the group on the way (the words
// mask[row][later chunk of the group], one per lane, were loaded while the previous group was being finished: one wave-wide OR per
// pair of chunks) -- then all 16 waves OR the group's kept rows (~40) into the LDS-resident "removed" bit vector for
// the columns behind the group.  One pair of workgroup barriers and one round of global loads per FOUR chunks instead of per chunk:
// the walk was bound by exactly those (12000 boxes: 188 chunks x 1.9 us).
// valid (may be null): boxes with valid[i] == 0 start out removed -- they are never kept and, never being kept, never suppress
// anything: the result equals the sweep over the list with those boxes deleted, with indices into the ORIGINAL list (the
// min-size filter of functions/rpn_proposal.py:57-59 without a compaction pass or a host round trip for the new length)
// seg (may be null): segmented form, one workgroup per segment (see nms_mask_kernel): keep indices are local to the segment and go to
// keep + its first row, its count to num_out[segment].
constexpr int NMS_G = 4;

// OR of a 32-bit value over the 64 lanes of a wave (result wave-uniform): inclusive scan inside each row of 16 lanes with DPP row
// shifts, then the two row broadcasts of gfx9 wave64 -- 6 v_or with DPP operands instead of 6 dependent ds_bpermute round trips
__device__ __forceinline__ unsigned wave_or32(unsigned x) {
#if defined(__HIP_DEVICE_COMPILE__)
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);     // row_shr:1
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);     // row_shr:2
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);     // row_shr:4
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);     // row_shr:8   -> lane 15 of a row = the row's OR
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, true);     // row_bcast:15 into rows 1, 3
    x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, true);     // row_bcast:31 into rows 2, 3  -> lane 63 = all
    return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
#else
    return x;
#endif
}
__device__ __forceinline__ uint64_t wave_or64(const uint64_t v) {
    return ((uint64_t)wave_or32((unsigned)(v >> 32)) << 32) | (uint64_t)wave_or32((unsigned)v);
}

__global__ __launch_bounds__(1024) void nms_sweep_kernel(const uint64_t *__restrict__ mask, const int n_,
                                                        const int col_blocks_, int64_t *__restrict__ keep,
                                                        int64_t *__restrict__ num_out, const int max_keep,
                                                        const unsigned char *__restrict__ valid,
                                                        const long long *__restrict__ seg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    int n = n_, col_blocks = col_blocks_;
    if (seg) {
        const long long *d = seg + 3 * blockIdx.x;
        keep += d[0]; n = (int)d[1]; mask += d[2]; num_out += blockIdx.x;
        col_blocks = (n + 63) / 64;
        if (n == 0) { if (threadIdx.x == 0) num_out[0] = 0; return; }
    }
    uint64_t *remv = reinterpret_cast<uint64_t *>(smem_raw);  // [col_blocks]
    uint64_t *bcast = remv + col_blocks;                       // [NMS_G] kept masks of the group, [NMS_G]: stop flag
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    for (int i = tid; i < col_blocks; i += 1024) {
        uint64_t w = 0;
        if (valid) {
            const int lim = min(64, n - i * 64);
            for (int j = 0; j < lim; ++j) w |= (uint64_t)(valid[i * 64 + j] == 0) << j;
        }
        remv[i] = w;
    }
    if (tid <= NMS_G) bcast[tid] = 0;
    __syncthreads();

    int count = 0;  // kept so far (tracked redundantly by every thread)
    // wave 0: this lane's words of the group being resolved -- W[g][g2], g2 >= g: mask[(b0 + g) * 64 + lane][b0 + g2] (g2 == g: the
    // diagonal word) -- and of the next group (loaded underneath the current group's second phase)
    uint64_t W[NMS_G][NMS_G], Wn[NMS_G][NMS_G];
    auto load_group = [&](const int b0, uint64_t (&D)[NMS_G][NMS_G]) {
#pragma unroll
        for (int g = 0; g < NMS_G; ++g)
#pragma unroll
            for (int g2 = g; g2 < NMS_G; ++g2) {
                const int row = (b0 + g) * 64 + lane, cb = b0 + g2;
                D[g][g2] = (cb < col_blocks && row < n) ? mask[(size_t)row * col_blocks + cb] : 0;
            }
    };
    if (tid < 64) load_group(0, W);

    for (int b0 = 0; b0 < col_blocks; b0 += NMS_G) {
        const int gn = min(NMS_G, col_blocks - b0);       // chunks of this group
        if (tid < 64) {
            if (b0 + NMS_G < col_blocks) load_group(b0 + NMS_G, Wn);
            uint64_t near[NMS_G];       // what the group's own kept rows remove in its later chunks (wave-uniform)
#pragma unroll
            for (int g = 0; g < NMS_G; ++g) near[g] = 0;
            bool stop = false;
#pragma unroll
            for (int g = 0; g < NMS_G; ++g) {
                uint64_t kept = 0;
                if (g < gn && !stop) {
                    const int base = (b0 + g) * 64;
                    const int size = min(n - base, 64);
                    const uint64_t removed = remv[b0 + g];
                    // `removed` is the same in every lane (one LDS word): make that explicit so the loop runs on the scalar unit
                    const uint64_t removed_u = (((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(removed >> 32)) << 32) |
                                                (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)removed)) | near[g];
                    uint64_t cand = ~removed_u;
                    if (size < 64) cand &= (1ULL << size) - 1ULL;
                    // The greedy decisions of a chunk as a FIXPOINT instead of a box-by-box recurrence: K <- cand & ~OR{D[j] : j in K},
                    // started at K = cand.  D[j] only has bits above j, so after t rounds the decisions of boxes 0 .. t are final (by
                    // induction: box i's decision depends on kept boxes j < i only), a K that reproduces itself satisfies the greedy
                    // equations, and those have exactly one solution -- the sequential sweep's.  Rounds needed = the longest chain
                    // "kept box suppresses a box that would have suppressed ..." + 1: 2 - 5 on RPN proposals, against one ~360-cycle
                    // scalar readlane step per KEPT box before (10 - 60 per chunk: that recurrence was 80 % of the sweep's time).
                    const uint64_t dg = W[g][g];
                    uint64_t K = cand;
                    for (int round = 0; round < 66; ++round) {
                        const uint64_t S = wave_or64(((K >> lane) & 1ULL) ? dg : 0ULL);
                        const uint64_t Kn = cand & ~S;
                        if (Kn == K) break;
                        K = Kn;
                    }
                    kept = K;
#pragma unroll
                    for (int g2 = g + 1; g2 < NMS_G; ++g2)       // what this chunk's kept rows remove in the group's later chunks
                        near[g2] |= wave_or64(((kept >> lane) & 1ULL) ? W[g][g2] : 0ULL);
                    // truncate to max_keep (indices are emitted in ascending order)
                    int nk = __popcll(kept);
                    if (max_keep > 0 && count + nk > max_keep) {
                        int allow = max_keep - count;
                        uint64_t k2 = kept, out = 0;
                        for (int c = 0; c < allow; ++c) { uint64_t low = k2 & (~k2 + 1); out |= low; k2 ^= low; }
                        kept = out;
                        nk = allow;
                    }
                    if ((kept >> lane) & 1ULL) {
                        int pos = count + __popcll(kept & ((1ULL << lane) - 1ULL));
                        keep[pos] = base + lane;
                    }
                    count += nk;
                    if (max_keep > 0 && count >= max_keep) stop = true;
                }
                if (lane == 0) bcast[g] = kept;
            }
            if (lane == 0) bcast[NMS_G] = stop ? 1 : 0;
#pragma unroll
            for (int g = 0; g < NMS_G; ++g)
#pragma unroll
                for (int g2 = g; g2 < NMS_G; ++g2) W[g][g2] = Wn[g][g2];
        }
        __syncthreads();
        uint64_t kept[NMS_G];
        int total = 0;
#pragma unroll
        for (int g = 0; g < NMS_G; ++g) { kept[g] = bcast[g]; total += __popcll(kept[g]); }
        const bool stop = bcast[NMS_G] != 0;
        if (tid >= 64) count += total;      // (wave 0 counted while it resolved)
        if (stop) break;
        // OR the group's kept rows into remv for the columns BEHIND the group.  16 waves: thread group grp = tid / 256 takes every
        // 4th kept row (ranked over the whole group), 8 independent row loads in flight per thread, groups merge through LDS atomics
        if (total && b0 + NMS_G < col_blocks) {
            const int grp = tid >> 8, t = tid & 255;
            for (int cb = b0 + NMS_G + t; cb < col_blocks; cb += 256) {
                uint64_t acc = 0;
                int rank = 0;
#pragma unroll
                for (int g = 0; g < NMS_G; ++g) {
                    uint64_t k = kept[g], mine = 0;   // the kept bits of chunk g this thread group owns
                    while (k) { const uint64_t low = k & (~k + 1); if ((rank & 3) == grp) mine |= low; k ^= low; ++rank; }
                    const size_t base = (size_t)(b0 + g) * 64;
                    while (mine) {
                        uint64_t v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            v[u] = 0;
                            if (mine) {
                                const int j = __ffsll((long long)mine) - 1;
                                mine &= mine - 1;
                                v[u] = mask[(base + j) * col_blocks + cb];
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) acc |= v[u];
                    }
                }
                if (acc) atomicOr(reinterpret_cast<unsigned long long *>(&remv[cb]), (unsigned long long)acc);
            }
        }
        __syncthreads();
    }
    if (tid == 0) num_out[0] = count;
}

// ---------------------------------------------------------------------------
// RoI max pooling.  Reference: extensions/_roi_pooling/src/roi_pooling_kernel.cu
// ---------------------------------------------------------------------------
struct RoiRect { int b, sw, sh, ew, eh; };

__device__ __forceinline__ RoiRect roi_rect(const float *roi, float scale) {
    RoiRect r;
    r.b = (int)roi[0];
    r.sw = (int)roundf(roi[1] * scale);  // half away from zero, roi_pooling_kernel.cu:46-49
    r.sh = (int)roundf(roi[2] * scale);
    r.ew = (int)roundf(roi[3] * scale);
    r.eh = (int)roundf(roi[4] * scale);
    return r;
}

// One thread per output element (n,c,ph,pw); consecutive threads write
// consecutive outputs (coalesced 2x 4B streams: value + argmax).  The feature
// map of config 2 is 4 MB and stays L2-resident, so the window scans hit cache.
__global__ __launch_bounds__(256) void roi_pool_fwd_kernel(const long long total, const float *__restrict__ feat,
                                                           const float scale, const int C, const int H, const int W,
                                                           const int PH, const int PW,
                                                           const float *__restrict__ rois, float *__restrict__ out,
                                                           int32_t *__restrict__ argmax) {
    for (long long index = blockIdx.x * (long long)blockDim.x + threadIdx.x; index < total;
         index += (long long)blockDim.x * gridDim.x) {
        const int pw = (int)(index % PW);
        const int ph = (int)((index / PW) % PH);
        const int c = (int)((index / PW / PH) % C);
        const int n = (int)(index / PW / PH / C);
        const RoiRect r = roi_rect(rois + (size_t)n * 5, scale);
        const int roi_w = (int)fmaxf((float)(r.ew - r.sw + 1), 1.f);
        const int roi_h = (int)fmaxf((float)(r.eh - r.sh + 1), 1.f);
        const float bin_h = __fdiv_rn((float)roi_h, (float)PH);
        const float bin_w = __fdiv_rn((float)roi_w, (float)PW);
        int hstart = (int)floorf((float)ph * bin_h);
        int wstart = (int)floorf((float)pw * bin_w);
        int hend = (int)ceilf((float)(ph + 1) * bin_h);
        int wend = (int)ceilf((float)(pw + 1) * bin_w);
        hstart = min(max(hstart + r.sh, 0), H);
        hend = min(max(hend + r.sh, 0), H);
        wstart = min(max(wstart + r.sw, 0), W);
        wend = min(max(wend + r.sw, 0), W);
        const bool empty = (hend <= hstart) || (wend <= wstart);
        float maxval = empty ? 0.f : -FLT_MAX;
        int maxidx = -1;
        const int base = (r.b * C + c) * H * W;
        for (int h = hstart; h < hend; ++h)
            for (int w = wstart; w < wend; ++w) {
                const int idx = base + h * W + w;
                const float v = feat[idx];
                if (v > maxval) { maxval = v; maxidx = idx; }
            }
        out[index] = maxval;
        if (argmax) argmax[index] = maxidx;
    }
}

// The same operator with the index arithmetic taken off the vector unit (round 6).  The form above spends its time on six 64-bit
// divisions by run-time values and a re-derivation of the RoI's rectangle per OUTPUT element (12.8 M of them at 512 RoIs x 512
// channels x 7 x 7: 80 us for 103 MB of stores = 1.3 TB/s).  Here a workgroup belongs to ONE RoI (blockIdx.y): the rectangle is
// wave-uniform (scalar loads, computed once), a thread's (ph, pw) bin is fixed for its whole life (256 threads walk the RoI's C * PH * PW
// outputs in steps of 256: with PH * PW = 49 the bin of thread t repeats every 49 steps, so it is simply recomputed with 32-bit
// constant-divisor arithmetic), and the output index is n * C * PH * PW + e: consecutive threads, consecutive outputs.  Same
// comparisons in the same scan order: bit-identical values and argmax.
template <int TPH, int TPW>      // > 0: the pooled size as compile-time constants (7 x 7: the detector's head)
__global__ __launch_bounds__(256) void roi_pool_fwd_roi_kernel(const float *__restrict__ feat, const float scale, const int C,
                                                               const int H, const int W, const int PH_arg, const int PW_arg,
                                                               const float *__restrict__ rois, float *__restrict__ out,
                                                               int32_t *__restrict__ argmax) {
    const int PH = TPH > 0 ? TPH : PH_arg, PW = TPW > 0 ? TPW : PW_arg;
    const int n = blockIdx.y;
    const RoiRect r = roi_rect(rois + (size_t)n * 5, scale);
    const int roi_w = (int)fmaxf((float)(r.ew - r.sw + 1), 1.f);
    const int roi_h = (int)fmaxf((float)(r.eh - r.sh + 1), 1.f);
    const float bin_h = __fdiv_rn((float)roi_h, (float)PH);
    const float bin_w = __fdiv_rn((float)roi_w, (float)PW);
    const int phw = PH * PW;
    const int per_roi = C * phw;
    const size_t obase = (size_t)n * per_roi;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < per_roi; e += gridDim.x * 256) {
        const int c = e / phw, rem = e - c * phw;
        const int ph = rem / PW, pw = rem - ph * PW;
        int hstart = (int)floorf((float)ph * bin_h);
        int wstart = (int)floorf((float)pw * bin_w);
        int hend = (int)ceilf((float)(ph + 1) * bin_h);
        int wend = (int)ceilf((float)(pw + 1) * bin_w);
        hstart = min(max(hstart + r.sh, 0), H);
        hend = min(max(hend + r.sh, 0), H);
        wstart = min(max(wstart + r.sw, 0), W);
        wend = min(max(wend + r.sw, 0), W);
        const bool empty = (hend <= hstart) || (wend <= wstart);
        float maxval = empty ? 0.f : -FLT_MAX;
        int maxidx = -1;
        const int base = (r.b * C + c) * H * W;
        for (int h = hstart; h < hend; ++h)
            for (int w = wstart; w < wend; ++w) {
                const int idx = base + h * W + w;
                const float v = feat[idx];
                if (v > maxval) { maxval = v; maxidx = idx; }
            }
        out[obase + e] = maxval;
        if (argmax) argmax[obase + e] = maxidx;
    }
}

// Backward, gather form with the reference's summation order (roi, ph, pw ascending) so the fp32 sums are
// bit-identical.  One workgroup = one (image, channel, 4-row band) of the feature map: it first compacts, in RoI order,
// the RoIs of that image whose integer rectangle touches the band (ballot + prefix count, order preserving) into LDS,
// then every thread walks only that short list.  The reference tests all R RoIs for every one of the B*C*H*W
// elements; here the band filter removes ~80-90 % of them before the per-element loop.
constexpr int kBandRows = 4;

__global__ __launch_bounds__(256) void roi_pool_bwd_kernel(const float *__restrict__ top,
                                                           const int32_t *__restrict__ argmax, const int R,
                                                           const float scale, const int C, const int H, const int W,
                                                           const int PH, const int PW, float *__restrict__ bottom,
                                                           const float *__restrict__ rois) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    int *rect = reinterpret_cast<int *>(smem_raw);   // [count][5]: roi index, sw, sh, ew, eh (only RoIs touching the band)
    __shared__ int s_count;
    __shared__ int s_wave_cnt[4];
    const int bands = (H + kBandRows - 1) / kBandRows;
    const int band = blockIdx.x % bands;
    const int c = (blockIdx.x / bands) % C;
    const int n = blockIdx.x / bands / C;
    const int h0 = band * kBandRows, h1 = min(H, h0 + kBandRows) - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int count = 0;
    for (int r0 = 0; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        bool hit = false;
        RoiRect q;
        q.b = q.sw = q.sh = q.ew = q.eh = 0;
        if (r < R) {
            q = roi_rect(rois + (size_t)r * 5, scale);
            hit = q.b == n && q.sh <= h1 && q.eh >= h0 && q.sw <= W - 1 && q.ew >= 0;
        }
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = count;
        for (int w2 = 0; w2 < wave; ++w2) before += s_wave_cnt[w2];
        if (hit) {
            const int pos = before + __popcll(bal & ((1ULL << lane) - 1ULL));
            rect[pos * 5 + 0] = r; rect[pos * 5 + 1] = q.sw; rect[pos * 5 + 2] = q.sh; rect[pos * 5 + 3] = q.ew; rect[pos * 5 + 4] = q.eh;
        }
        count += s_wave_cnt[0] + s_wave_cnt[1] + s_wave_cnt[2] + s_wave_cnt[3];
        __syncthreads();
    }
    if (tid == 0) s_count = count;
    __syncthreads();
    count = s_count;

    const int bins = PH * PW;
    for (int e = tid; e < kBandRows * W; e += 256) {
        const int h = h0 + e / W, w = e % W;
        if (h >= H) continue;
        const int index = ((n * C + c) * H + h) * W + w;
        float g = 0.f;
        for (int i = 0; i < count; ++i) {
            const int *q = rect + i * 5;  // uniform address: LDS broadcast
            const int sw = q[1], sh = q[2], ew = q[3], eh = q[4];
            if (!(w >= sw && w <= ew && h >= sh && h <= eh)) continue;
            const int roi_w = (int)fmaxf((float)(ew - sw + 1), 1.f);
            const int roi_h = (int)fmaxf((float)(eh - sh + 1), 1.f);
            const float bin_h = __fdiv_rn((float)roi_h, (float)PH);
            const float bin_w = __fdiv_rn((float)roi_w, (float)PW);
            int phs = (int)floorf(__fdiv_rn((float)(h - sh), bin_h));
            int phe = (int)ceilf(__fdiv_rn((float)(h - sh + 1), bin_h));
            int pws = (int)floorf(__fdiv_rn((float)(w - sw), bin_w));
            int pwe = (int)ceilf(__fdiv_rn((float)(w - sw + 1), bin_w));
            phs = min(max(phs, 0), PH); phe = min(max(phe, 0), PH);
            pws = min(max(pws, 0), PW); pwe = min(max(pwe, 0), PW);
            const size_t off = ((size_t)q[0] * C + c) * bins;
            for (int ph = phs; ph < phe; ++ph)
                for (int pw = pws; pw < pwe; ++pw) {
                    const size_t o = off + ph * PW + pw;
                    if (argmax[o] == index) g += top[o];
                }
        }
        bottom[index] = g;
    }
}

// Backward, ORDERED SCATTER form (the one the C ABI launches when PH*PW <= 64 and a plane fits in LDS).
// The gradient of one (image, channel) plane is the sum, over (roi, ph, pw) in ascending order, of top[roi,c,ph,pw] at
// pixel argmax[roi,c,ph,pw] -- exactly what the reference's gather loop adds up, in its order.  One WAVE owns one plane,
// kept in LDS; lane = bin.  (Eight waves share a plane, each owning a contiguous eighth of its pixels and ignoring the
// bins that land elsewhere: 8x the waves to hide the LDS round-trip chain, and most RoIs miss most slices.)  For each RoI (ascending) the wave reads its 49 argmax/top values with two coalesced loads and
// adds them into the plane.  Bins of one RoI can share a pixel (floor/ceil bin edges overlap; tiny RoIs collapse onto one
// pixel), and fp32 addition order matters, so equal targets are serialised lowest-bin-first: every pending lane posts its
// lane id with an LDS atomicMin on a tag word of its pixel, the lane that finds its own id there adds and retires, the
// rest go round again (1 round unless bins collide).  No divisions per bin edge, argmax/top read exactly once
// (~100 MB for 512 RoIs x 512 channels).  The gather kernel above remains the fallback.
// The reference's gather (roi_pooling_kernel.cu:161-166) only looks at RoIs whose rounded rectangle [sw..ew] x [sh..eh] holds the
// pixel, and the forward's last bin can end one pixel PAST that rectangle (fl(roi / 7) * 7 rounds up for extents 57, 114, 121, 228,
// ...): an argmax there gets no gradient in the reference.  The same gate is applied here when a RoI is staged, which is what
// makes this form bit-identical to the gather kernel (tests/test_roi_edges_gpu.py sweeps the extents).
constexpr int kScatterBands = 8;   // waves per plane
constexpr int kScatterChunk = 32;  // RoIs staged per step

// Round 3: the eight band-waves of a plane no longer each read every RoI's argmax / top values from global memory (8 x 100 MB through
// L2, and a dependent global round trip per 8 RoIs and wave: 410 us).  The workgroup stages kScatterChunk RoIs at a time into LDS --
// 512 threads x 4 entries, the loads of chunk i+1 in flight while chunk i is scattered -- and every wave scans the chunk there.
__global__ __launch_bounds__(64 * kScatterBands) void roi_pool_bwd_scatter_kernel(const float *__restrict__ top,
                                                                                 const int32_t *__restrict__ argmax,
                                                                                 const float *__restrict__ rois, const int R,
                                                                                 const int C, const int HW, const int bins,
                                                                                 float *__restrict__ bottom, const float scale,
                                                                                 const int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;                   // plane = n * C + c
    const int n = p / C, c = p - n * C;
    // this wave's slice of the plane: pixels [lo, hi)
    const int per = (HW + kScatterBands - 1) / kScatterBands;
    const int lo = wave * per, hi = min(HW, lo + per);
    float *plane = reinterpret_cast<float *>(smem_raw) + (size_t)wave * per * 2;
    int *tag = reinterpret_cast<int *>(plane + per);
    // staging buffers behind the planes: [2][kScatterChunk][64] of (argmax relative to the plane, top)
    int *st_a = reinterpret_cast<int *>(smem_raw + (size_t)kScatterBands * per * 8);
    float *st_g = reinterpret_cast<float *>(st_a + 2 * kScatterChunk * 64);
    for (int i = lane; i < per; i += 64) { plane[i] = 0.f; tag[i] = 64; }
    const int pbase = p * HW;
    const int base = pbase + lo, span = hi - lo;
    constexpr int E = kScatterChunk * 64 / (64 * kScatterBands);   // entries per thread and chunk
    int ra[E];
    float rg[E];
    auto fetch = [&](const int r0) {
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int e = tid + k * 64 * kScatterBands, r = r0 + (e >> 6), l = e & 63;
            ra[k] = -1;
            rg[k] = 0.f;
            if (r < R && l < bins) {
                // r is the same in all 64 lanes (e >> 6): one rectangle per staged RoI, not per bin
                const RoiRect q = roi_rect(rois + (size_t)r * 5, scale);
                if (q.b == n) {
                    const size_t o = ((size_t)r * C + c) * bins + l;
                    const int a = argmax[o] - pbase;
                    if (a >= 0) {      // (-1 = empty bin; argmax of a RoI of image n lies in plane p)
                        const int h = a / W, w = a - h * W;
                        if (w >= q.sw && w <= q.ew && h >= q.sh && h <= q.eh) { ra[k] = a; rg[k] = top[o]; }
                    }
                }
            }
        }
    };
    auto stash = [&](const int buf) {
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int e = tid + k * 64 * kScatterBands;
            st_a[buf * kScatterChunk * 64 + e] = ra[k];
            st_g[buf * kScatterChunk * 64 + e] = rg[k];
        }
    };
    fetch(0);
    stash(0);
    __syncthreads();
    int cur = 0;
    for (int r0 = 0; r0 < R; r0 += kScatterChunk) {
        const bool more = r0 + kScatterChunk < R;
        if (more) fetch(r0 + kScatterChunk);             // global loads in flight while this chunk is scattered
        // rows beyond R are staged as "no target", so a chunk is always walked whole: four RoIs' staged values are read ahead of the
        // serial scatter rounds (their LDS latency would otherwise be paid per RoI, in front of every round)
        constexpr int UA = 4;
        for (int u0 = 0; u0 < kScatterChunk; u0 += UA) {
            int av[UA];
            float gvv[UA];
#pragma unroll
            for (int k = 0; k < UA; ++k) {
                av[k] = st_a[(cur * kScatterChunk + u0 + k) * 64 + lane];
                gvv[k] = st_g[(cur * kScatterChunk + u0 + k) * 64 + lane];
            }
#pragma unroll
            for (int k = 0; k < UA; ++k) {
                const int a = av[k] - lo;
                const float gv = gvv[k];
                bool pending = av[k] >= 0 && a >= 0 && a < span;
                const int ix = pending ? a : 0;
                while (__ballot(pending)) {
                    if (pending) atomicMin(&tag[ix], lane);
                    if (pending && tag[ix] == lane) {
                        atomicAdd(&plane[ix], gv);   // ONE LDS operation (ds_add_f32): this lane is the only writer of the pixel now
                        tag[ix] = 64;
                        pending = false;
                    }
                }
            }
            // (scattering the four RoIs of a read-ahead group TOGETHER -- rank = RoI-in-group * 64 + bin on the pixel tags -- was built
            // and is bit-identical, but slower: 332 vs 273 us; overlapping RoIs share their argmax pixels, so the rounds do not shrink)
        }
        if (more) stash(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    for (int i = lane; i < span; i += 64) bottom[(size_t)base + i] = plane[i];
}

// ---------------------------------------------------------------------------
// RoIAlign (old single-sample form).  Reference: extensions/_roi_align/src/roi_align_kernel.cu
// The reference mixes float and double literals; the double sub-expressions are
// kept in double so roundings happen where nvcc placed them.
// ---------------------------------------------------------------------------
struct RaPoint { bool ok; int upleft; float hr, wr; };

__device__ __forceinline__ RaPoint ra_point(const float *roi, float scale, int C, int H, int W, int AH, int AW, int c,
                                            int ph, int pw) {
    RaPoint p; p.ok = false; p.upleft = 0; p.hr = p.wr = 0.f;
    const float bi = roi[0];
    const float sw = roi[1] * scale, sh = roi[2] * scale, ew = roi[3] * scale, eh = roi[4] * scale;
    const float roi_w = fmaxf((float)((double)(ew - sw) + 1.), 0.f);
    const float roi_h = fmaxf((float)((double)(eh - sh) + 1.), 0.f);
    const float bin_h = (float)((double)roi_h / ((double)AH - 1.));
    const float bin_w = (float)((double)roi_w / ((double)AW - 1.));
    const float h = (float)ph * bin_h + sh;
    const float w = (float)pw * bin_w + sw;
    const int hstart = (int)fminf(floorf(h), (float)(H - 2));
    const int wstart = (int)fminf(floorf(w), (float)(W - 2));
    const int img_start = (int)(bi * (float)(C * H * W));
    if (h < 0 || h >= H || w < 0 || w >= W) return p;
    p.ok = true;
    p.hr = h - (float)hstart;
    p.wr = w - (float)wstart;
    p.upleft = img_start + (c * H + hstart) * W + wstart;
    return p;
}

__global__ __launch_bounds__(256) void roi_align_fwd_kernel(const long long total, const float *__restrict__ feat,
                                                            const float scale, const int C, const int H, const int W,
                                                            const int AH, const int AW, const float *__restrict__ rois,
                                                            float *__restrict__ out, const int R, const int cmajor) {
    // cmajor: the output is [C][R][AH][AW] (channel-major RoI-head layout) instead of [R][C][AH][AW]; index runs over the output
    for (long long index = blockIdx.x * (long long)blockDim.x + threadIdx.x; index < total;
         index += (long long)blockDim.x * gridDim.x) {
        const int pw = (int)(index % AW);
        const int ph = (int)((index / AW) % AH);
        const int c = cmajor ? (int)(index / AW / AH / R) : (int)((index / AW / AH) % C);
        const int n = cmajor ? (int)((index / AW / AH) % R) : (int)(index / AW / AH / C);
        const RaPoint p = ra_point(rois + (size_t)n * 5, scale, C, H, W, AH, AW, c, ph, pw);
        if (!p.ok) { out[index] = 0.f; continue; }
        const double hr = p.hr, wr = p.wr;
        const double v = (double)feat[p.upleft] * (1. - hr) * (1. - wr) + (double)feat[p.upleft + 1] * (1. - hr) * wr +
                         (double)feat[p.upleft + W] * hr * (1. - wr) + (double)feat[p.upleft + W + 1] * hr * wr;
        out[index] = (float)v;
    }
}

__global__ __launch_bounds__(256) void roi_align_bwd_kernel(const long long total, const float *__restrict__ top,
                                                            const float scale, const int C, const int H, const int W,
                                                            const int AH, const int AW, float *__restrict__ bottom,
                                                            const float *__restrict__ rois, const int R, const int cmajor) {
    for (long long index = blockIdx.x * (long long)blockDim.x + threadIdx.x; index < total;
         index += (long long)blockDim.x * gridDim.x) {
        const int pw = (int)(index % AW);
        const int ph = (int)((index / AW) % AH);
        const int c = cmajor ? (int)(index / AW / AH / R) : (int)((index / AW / AH) % C);
        const int n = cmajor ? (int)((index / AW / AH) % R) : (int)(index / AW / AH / C);
        const RaPoint p = ra_point(rois + (size_t)n * 5, scale, C, H, W, AH, AW, c, ph, pw);
        if (!p.ok) continue;
        const double hr = p.hr, wr = p.wr, d = top[index];
        atomicAdd(bottom + p.upleft, (float)(d * (1. - hr) * (1 - wr)));
        atomicAdd(bottom + p.upleft + 1, (float)(d * (1. - hr) * wr));
        atomicAdd(bottom + p.upleft + W, (float)(d * hr * (1 - wr)));
        atomicAdd(bottom + p.upleft + W + 1, (float)(d * hr * wr));
    }
}

// Plane-resident form of the backward: one workgroup owns one (image, channel) plane of the gradient, keeps it in LDS, walks
// every RoI of that image (thread = one bin; 256 / (AH*AW) RoIs in flight) and adds the four bilinear corners with LDS
// atomics (ds_add_f32), then adds the plane to the output once.  The global-atomic form above sends 4 x R x C x AH x AW float
// atomics to the L2 (512 RoIs x 1024 channels x 8 x 8: 134 M atomics, 2.7 ms on the ResNet-50 C4 head); here the L2 sees one
// coalesced read of the top gradient and one read-modify-write of the plane.
__global__ __launch_bounds__(256) void roi_align_bwd_plane_kernel(const float *__restrict__ top, const int R, const float scale,
                                                                  const int C, const int H, const int W, const int AH,
                                                                  const int AW, float *__restrict__ bottom,
                                                                  const float *__restrict__ rois, const int cmajor) {
    extern __shared__ float plane[];
    const int c = blockIdx.x % C, b = blockIdx.x / C;
    const int hw = H * W, bins = AH * AW;
    for (int i = threadIdx.x; i < hw; i += 256) plane[i] = 0.f;
    __syncthreads();
    const int per = 256 / bins;                     // RoIs in flight (bins <= 256, checked by the launcher)
    const int sub = threadIdx.x / bins, bin = threadIdx.x - sub * bins;
    const int ph = bin / AW, pw = bin - ph * AW;
    const int plane_base = (b * C + c) * hw;
    if (sub < per) {
        for (int n = sub; n < R; n += per) {
            const float *roi = rois + (size_t)n * 5;
            if ((int)roi[0] != b) continue;
            const RaPoint p = ra_point(roi, scale, C, H, W, AH, AW, c, ph, pw);
            if (!p.ok) continue;
            const double hr = p.hr, wr = p.wr, d = top[(cmajor ? (size_t)c * R + n : (size_t)n * C + c) * bins + bin];
            const int o = p.upleft - plane_base;
            atomicAdd(plane + o, (float)(d * (1. - hr) * (1 - wr)));
            atomicAdd(plane + o + 1, (float)(d * (1. - hr) * wr));
            atomicAdd(plane + o + W, (float)(d * hr * (1 - wr)));
            atomicAdd(plane + o + W + 1, (float)(d * hr * wr));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < hw; i += 256) bottom[(size_t)plane_base + i] += plane[i];
}

// ---------------------------------------------------------------------------
// Focal loss.  Reference: extensions/_focal_loss/src/cuda/focal_loss_{sigmoid,softmax}_kernel.cu
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void focal_sigmoid_fwd_kernel(const int N, const float *__restrict__ logits,
                                                                const int32_t *__restrict__ targets,
                                                                const float weight_pos, const float gamma,
                                                                const float alpha, const int num_classes,
                                                                float *__restrict__ losses) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += blockDim.x * gridDim.x) {
        const int d = i % num_classes;
        const int t = targets[i / num_classes];
        const float c1 = (t == (d + 1));
        const float c2 = ((t != -1) & (t != (d + 1)));
        const float Np = (float)fmax((double)weight_pos, 1.0);
        const float zn = (float)((1.0 - (double)alpha) / (double)Np);
        const float zp = alpha / Np;
        const float x = logits[i];
        const float p = (float)(1. / (1. + (double)expf(-x)));
        const float term1 = (float)((double)powf((float)(1. - (double)p), gamma) * (double)logf(fmaxf(p, FLT_MIN)));
        const float ge = (x >= 0);
        const float term2 =
            (float)((double)powf(p, gamma) *
                    (-1. * (double)x * (double)ge -
                     (double)logf((float)(1. + (double)expf((float)((double)x - 2. * (double)x * (double)ge))))));
        float l = 0.0f;
        l += -c1 * term1 * zp;
        l += -c2 * term2 * zn;
        losses[i] = l;
    }
}

__global__ __launch_bounds__(256) void focal_sigmoid_bwd_kernel(const int N, const float *__restrict__ logits,
                                                                const int32_t *__restrict__ targets,
                                                                float *__restrict__ dX, const float weight_pos,
                                                                const float gamma, const float alpha,
                                                                const int num_classes) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += blockDim.x * gridDim.x) {
        const int d = i % num_classes;
        const int t = targets[i / num_classes];
        const float Np = (float)fmax((double)weight_pos, 1.0);
        const float zn = (float)((1.0 - (double)alpha) / (double)Np);
        const float zp = alpha / Np;
        const float c1 = (t == (d + 1));
        const float c2 = ((t != -1) & (t != (d + 1)));
        const float x = logits[i];
        const float p = (float)(1. / (1. + (double)expf(-x)));
        const float term1 = (float)((double)powf((float)(1. - (double)p), gamma) *
                                    (1. - (double)p - (double)(p * gamma * logf(fmaxf(p, FLT_MIN)))));
        const float ge = (x >= 0);
        const double lg = -1. * (double)x * (double)ge -
                          (double)logf((float)(1. + (double)expf((float)((double)x - 2. * (double)x * (double)ge))));
        const float term2 = (float)((double)powf(p, gamma) * (lg * (1. - (double)p) * (double)gamma - (double)p));
        float g = 0.0f;
        g += -c1 * zp * term1;
        g += -c2 * zn * term2;
        dX[i] = g;
    }
}

// softmax + per-row loss fused in one pass (the reference launches two kernels)
__global__ __launch_bounds__(256) void focal_softmax_fwd_kernel(const int rows, const float *__restrict__ X,
                                                                const int32_t *__restrict__ targets,
                                                                const float weight_pos, const float gamma,
                                                                const float alpha, const int num_classes,
                                                                float *__restrict__ losses, float *__restrict__ P) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += blockDim.x * gridDim.x) {
        const int base = r * num_classes;
        float mx = -FLT_MAX;
        for (int c = 0; c < num_classes; ++c) mx = fmaxf(mx, X[base + c]);
        float es = 0.0f;
        for (int c = 0; c < num_classes; ++c) { float e = expf(X[base + c] - mx); P[base + c] = e; es += e; }
        for (int c = 0; c < num_classes; ++c) P[base + c] = __fdiv_rn(P[base + c], es);
        const int label = targets[r];
        const float Np = (float)fmax((double)weight_pos, 1.0);
        const float z = (label == 0) * (1 - alpha) / Np + (label >= 1) * alpha / Np;
        float l = 0.0f;
        if (label >= 0) {
            const float pl = P[base + label];
            l = -(powf((float)(1.0 - (double)pl), gamma) * logf(fmaxf(pl, FLT_MIN))) * z;
        }
        losses[r] = l;
    }
}

__global__ __launch_bounds__(256) void focal_softmax_bwd_weight_kernel(const int rows, const float *__restrict__ P,
                                                                       const int32_t *__restrict__ targets,
                                                                       float *__restrict__ buff,
                                                                       const float weight_pos, const float gamma,
                                                                       const float alpha, const int num_classes) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += blockDim.x * gridDim.x) {
        const int base = r * num_classes, label = targets[r];
        const float Np = (float)fmax((double)weight_pos, 1.0);
        const float z = (label == 0) * (1 - alpha) / Np + (label >= 1) * alpha / Np;
        float b = 0.0f;
        if (label >= 0) {
            const float onemp = (float)(1. - (double)P[base + label]);
            const float p = P[base + label];
            // p == 1 (logf == 0, onemp == 0): the second term is gamma * 0^(gamma - 1) * 0, i.e. 0 * inf = NaN for gamma < 1 (a softmax
            // rounds to exactly 1 in fp32 from a logit gap of about 17; with one class always).  Its limit is 0, which is also what
            // the expression gives for every gamma >= 1: same bits wherever the reference's value is a number.
            const float lg = logf(fmaxf(p, FLT_MIN));
            const float second = lg == 0.f ? 0.f : gamma * powf(onemp, gamma - 1) * p * lg;
            b = (-powf(onemp, gamma) + second) * z;
        }
        buff[r] = b;
    }
}

__global__ __launch_bounds__(256) void focal_softmax_bwd_kernel(const int N, const float *__restrict__ P,
                                                                const int32_t *__restrict__ targets,
                                                                const float *__restrict__ buff,
                                                                float *__restrict__ dX, const int num_classes) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += blockDim.x * gridDim.x) {
        const int ind = i / num_classes, cls = i % num_classes;
        const int label = targets[ind];
        const float c1 = (float)((label >= 0) * 1.0), c2 = (float)((label == cls) * 1.0);
        dX[i] = c1 * buff[ind] * (c2 - P[i]);
    }
}

// ---------------------------------------------------------------------------
// Box overlap matrices
// ---------------------------------------------------------------------------
// extensions/_bbox_helper/src/cuda/iou_overlap_kernel.cu:33-65
__global__ __launch_bounds__(256) void iou_overlaps_kernel(const float *__restrict__ b1, const float *__restrict__ b2,
                                                           const int sz, const int n1, const int n2,
                                                           float *__restrict__ out) {
    const long long total = (long long)n1 * n2;
    for (long long index = blockIdx.x * (long long)blockDim.x + threadIdx.x; index < total;
         index += (long long)blockDim.x * gridDim.x) {
        const int i = (int)(index / n2), j = (int)(index % n2);
        const float *p = b1 + (size_t)i * sz, *q = b2 + (size_t)j * sz;
        const float a1 = (p[2] - p[0]) * (p[3] - p[1]), a2 = (q[2] - q[0]) * (q[3] - q[1]);
        const float left = fmaxf(p[0], q[0]), right = fminf(p[2], q[2]);
        const float top = fmaxf(p[1], q[1]), bottom = fminf(p[3], q[3]);
        const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
        const float interS = width * height;
        const float unionS = fmaxf(a1 + a2 - interS, 1.0f);
        out[index] = __fdiv_rn(interS, unionS);
    }
}

// extensions/_cython_bbox/cython_bbox.pyx:32-73
__global__ __launch_bounds__(256) void bbox_overlaps_kernel(const float *__restrict__ boxes, const int N,
                                                            const float *__restrict__ query, const int K,
                                                            float *__restrict__ out) {
    const long long total = (long long)N * K;
    for (long long index = blockIdx.x * (long long)blockDim.x + threadIdx.x; index < total;
         index += (long long)blockDim.x * gridDim.x) {
        const int n = (int)(index / K), k = (int)(index % K);
        const float *b = boxes + (size_t)n * 4, *q = query + (size_t)k * 4;
        const float box_area = (q[2] - q[0]) * (q[3] - q[1]);
        float o = 0.f;
        const float iw = fminf(b[2], q[2]) - fmaxf(b[0], q[0]);
        if (iw > 0) {
            const float ih = fminf(b[3], q[3]) - fmaxf(b[1], q[1]);
            if (ih > 0) {
                const float ua = (b[2] - b[0]) * (b[3] - b[1]) + box_area - iw * ih;
                o = __fdiv_rn(iw * ih, ua);
            }
        }
        out[index] = o;
    }
}

}  // namespace scda

using namespace scda;

// ============================= C ABI ========================================
SCDA_API int scda_version(void) { return 100; }

SCDA_API int scda_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

SCDA_API const char *scda_last_error(void) { return g_err; }

SCDA_API void scda_prof_enable(unsigned kernel_mask) { g_prof_mask = kernel_mask; }

// after a device synchronisation: per kernel class k (see scda_prof_kernel_name): launches, total milliseconds,
// total algorithmic FLOPs.  Arrays hold scda_prof_num_kernels() entries.  Clears the recorded events.
SCDA_API int scda_prof_num_kernels(void) { return PK_COUNT; }
SCDA_API const char *scda_prof_kernel_name(int k) {
    static const char *names[PK_COUNT] = {
        "conv_igemm_glds_kernel<128|256,*,3,3,1,fwd>", "conv_igemm_glds_kernel<128|256,*,3,3,2,fwd>", "conv_igemm_glds_kernel<128|256,*,1,1,1,fwd>",
        "conv_igemm_glds_kernel<64,*,3,3,1,fwd>", "conv_igemm_glds_kernel<64,*,3,3,2,fwd>", "conv_igemm_glds_kernel<64,*,1,1,1,fwd>",
        "conv_igemm_glds_kernel<128|256,*,3,3,1,dgrad>", "conv_igemm_glds_kernel<128|256,*,3,3,2,dgrad>", "conv_igemm_glds_kernel<128|256,*,1,1,1,dgrad>",
        "conv_igemm_glds_kernel<64,*,3,3,1,dgrad>", "conv_igemm_glds_kernel<64,*,3,3,2,dgrad>", "conv_igemm_glds_kernel<64,*,1,1,1,dgrad>",
        "conv_wgrad_glds_kernel<*,*,3,3,1>", "conv_wgrad_glds_kernel<*,*,3,3,2>", "conv_wgrad_glds_kernel<*,*,1,1,1>", "gemm_glds_kernel<*>", "conv_igemm_kernel<*>",
        "conv_wino_kernel<fwd>", "conv_wino_kernel<dgrad>", "conv_wino_wgrad_kernel"};
    return (k >= 0 && k < PK_COUNT) ? names[k] : "";
}
SCDA_API int scda_prof_collect(long long *launches, double *ms, double *flops, double *bytes) {
    for (int k = 0; k < PK_COUNT; ++k) { launches[k] = 0; ms[k] = 0; flops[k] = 0; if (bytes) bytes[k] = 0; }
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (auto &r : g_prof) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
            launches[r.kernel] += 1; ms[r.kernel] += t; flops[r.kernel] += r.flops;
            if (bytes) bytes[r.kernel] += r.bytes;
        } else {
            (void)hipGetLastError();
        }
        g_prof_pool.push_back(r.a); g_prof_pool.push_back(r.b);
    }
    g_prof.clear();
    return SCDA_OK;
}

SCDA_API size_t scda_nms_workspace_bytes(int n) {
    if (n <= 0) return 0;
    const size_t cb = (size_t)(n + 63) / 64;
    return (size_t)n * cb * sizeof(uint64_t);
}

SCDA_API int scda_nms_mask_hip(const float *boxes, int n, float thresh, uint64_t *mask, void *stream) {
    if (n < 0 || (n > 0 && (!boxes || !mask))) { set_error("scda_nms_mask_hip: bad arguments"); return SCDA_EINVAL; }
    if (n == 0) return SCDA_OK;
    const int cb = (n + 63) / 64;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(cb, cb), dim3(64), 0, as_stream(stream), n, thresh, boxes, mask, cb, (const long long *)nullptr);
    return launch_status("nms_mask_kernel");
}

SCDA_API int scda_nms_hip(const float *boxes, int n, float thresh, void *mask_ws, int64_t *keep, int64_t *num_out,
                          int max_keep, void *stream) {
    return scda_nms_valid_hip(boxes, nullptr, n, thresh, mask_ws, keep, num_out, max_keep, stream);
}

SCDA_API int scda_nms_valid_hip(const float *boxes, const unsigned char *valid, int n, float thresh, void *mask_ws, int64_t *keep,
                                int64_t *num_out, int max_keep, void *stream) {
    if (n < 0 || !num_out || (n > 0 && (!boxes || !mask_ws || !keep))) {
        set_error("scda_nms_hip: bad arguments");
        return SCDA_EINVAL;
    }
    if (n == 0) {
        hipError_t e = hipMemsetAsync(num_out, 0, sizeof(int64_t), as_stream(stream));
        return e == hipSuccess ? SCDA_OK : SCDA_ELAUNCH;
    }
    const int cb = (n + 63) / 64;
    int st = scda_nms_mask_hip(boxes, n, thresh, (uint64_t *)mask_ws, stream);
    if (st) return st;
    const size_t lds = (size_t)(cb + NMS_G + 1) * sizeof(uint64_t);
    if (lds > 64 * 1024) { set_error("scda_nms_hip: n=%d too large for the LDS-resident sweep", n); return SCDA_EINVAL; }
    hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(1024), lds, as_stream(stream), (const uint64_t *)mask_ws, n, cb,
                       keep, num_out, max_keep, valid, (const long long *)nullptr);
    return launch_status("nms_sweep_kernel");
}

// S independent score-sorted lists in ONE mask launch + ONE sweep launch (one workgroup per list): functions/predict_bbox.py:29-55
// calls nms once per (class, image).  seg: DEVICE int64 [S][3] = {first row of the list in boxes / keep, its length, first word of
// its mask in mask_ws (lengths n occupy n * ceil(n / 64) words)}; max_n = the longest list; keep [rows of all lists] receives each
// list's kept indices (local to the list) at its first row, num_out [S] the counts.
SCDA_API int scda_nms_segments_hip(const float *boxes, const long long *seg, int S, int max_n, float thresh, void *mask_ws, int64_t *keep,
                                   int64_t *num_out, void *stream) {
    if (S < 0 || max_n < 0 || (S > 0 && (!seg || !num_out)) || (S > 0 && max_n > 0 && (!boxes || !mask_ws || !keep))) {
        set_error("scda_nms_segments_hip: bad arguments");
        return SCDA_EINVAL;
    }
    if (S == 0) return SCDA_OK;
    if (max_n == 0) {
        hipError_t e = hipMemsetAsync(num_out, 0, sizeof(int64_t) * S, as_stream(stream));
        return e == hipSuccess ? SCDA_OK : SCDA_ELAUNCH;
    }
    const int cb = (max_n + 63) / 64;
    const size_t lds = (size_t)(cb + NMS_G + 1) * sizeof(uint64_t);
    if (lds > 64 * 1024 || S > 65535) { set_error("scda_nms_segments_hip: list of %d boxes / %d lists too large", max_n, S); return SCDA_EINVAL; }
    hipLaunchKernelGGL(nms_mask_kernel, dim3(cb, cb, S), dim3(64), 0, as_stream(stream), 0, thresh, boxes, (uint64_t *)mask_ws, 0, seg);
    int st = launch_status("nms_mask_kernel");
    if (st) return st;
    hipLaunchKernelGGL(nms_sweep_kernel, dim3(S), dim3(1024), lds, as_stream(stream), (const uint64_t *)mask_ws, 0, 0, keep, num_out, 0,
                       (const unsigned char *)nullptr, seg);
    return launch_status("nms_sweep_kernel");
}

SCDA_API int scda_roi_pool_fwd_hip(const float *features, const float *rois, int R, int B, int C, int H, int W, int PH,
                                   int PW, float spatial_scale, float *out, int32_t *argmax, void *stream) {
    if (R < 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || PH <= 0 || PW <= 0) { set_error("scda_roi_pool_fwd_hip: bad shape"); return SCDA_EINVAL; }
    if ((long long)B * C * H * W > 0x7fffffffLL) { set_error("scda_roi_pool_fwd_hip: features exceed int32 indexing"); return SCDA_EINVAL; }
    if (R == 0) return SCDA_OK;
    if (!features || !rois || !out) { set_error("scda_roi_pool_fwd_hip: null pointer"); return SCDA_EINVAL; }
    const long long total = (long long)R * C * PH * PW;
    // one block column per RoI; past the grid's y limit: one thread per output element, 64-bit index math
    if (R <= 65535 && (long long)C * PH * PW < (1LL << 30)) {
        const int per_roi = C * PH * PW;
        const dim3 grid((unsigned)std::min((per_roi + 255) / 256, 64), (unsigned)R);
        if (PH == 7 && PW == 7)
            hipLaunchKernelGGL((roi_pool_fwd_roi_kernel<7, 7>), grid, dim3(256), 0, as_stream(stream), features, spatial_scale, C, H, W, PH, PW, rois, out, argmax);
        else
            hipLaunchKernelGGL((roi_pool_fwd_roi_kernel<0, 0>), grid, dim3(256), 0, as_stream(stream), features, spatial_scale, C, H, W, PH, PW, rois, out, argmax);
        return launch_status("roi_pool_fwd_roi_kernel");
    }
    const int grid = (int)((total + 255) / 256 > 65536 * 4 ? 65536 * 4 : (total + 255) / 256);
    hipLaunchKernelGGL(roi_pool_fwd_kernel, dim3(grid), dim3(256), 0, as_stream(stream), total, features, spatial_scale,
                       C, H, W, PH, PW, rois, out, argmax);
    return launch_status("roi_pool_fwd_kernel");
}

SCDA_API int scda_roi_pool_bwd_hip(const float *top_grad, const int32_t *argmax, const float *rois, int R, int B, int C,
                                   int H, int W, int PH, int PW, float spatial_scale, float *bottom_grad,
                                   void *stream) {
    if (R < 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || PH <= 0 || PW <= 0 || !bottom_grad) { set_error("scda_roi_pool_bwd_hip: bad shape"); return SCDA_EINVAL; }
    const long long total = (long long)B * C * H * W;
    if (total > 0x7fffffffLL) { set_error("scda_roi_pool_bwd_hip: features exceed int32 indexing"); return SCDA_EINVAL; }
    if (R == 0) {
        hipError_t e = hipMemsetAsync(bottom_grad, 0, (size_t)total * sizeof(float), as_stream(stream));
        return e == hipSuccess ? SCDA_OK : SCDA_ELAUNCH;
    }
    if (!top_grad || !argmax || !rois) { set_error("scda_roi_pool_bwd_hip: null pointer"); return SCDA_EINVAL; }
    const size_t per = ((size_t)H * W + kScatterBands - 1) / kScatterBands;
    const size_t scatter_lds = per * 8 * kScatterBands + (size_t)2 * kScatterChunk * 64 * 8;
    // more than 64 KB of dynamic LDS must be asked for once per kernel; if the runtime refuses, the gather kernel below takes the shape
    static const bool big_lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(roi_pool_bwd_scatter_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) == hipSuccess;
    if (!big_lds_ok) (void)hipGetLastError();
    if (PH * PW <= 64 && scatter_lds <= (big_lds_ok ? 96 : 64) * (size_t)1024) {
        hipLaunchKernelGGL(roi_pool_bwd_scatter_kernel, dim3(B * C), dim3(64 * kScatterBands), scatter_lds, as_stream(stream),
                           top_grad, argmax, rois, R, C, H * W, PH * PW, bottom_grad, spatial_scale, W);
        return launch_status("roi_pool_bwd_scatter_kernel");
    }
    const size_t lds = (size_t)R * 5 * sizeof(int);
    if (lds > 64 * 1024) { set_error("scda_roi_pool_bwd_hip: R=%d too large", R); return SCDA_EINVAL; }
    const int bands = (H + kBandRows - 1) / kBandRows;
    hipLaunchKernelGGL(roi_pool_bwd_kernel, dim3((unsigned)((long long)B * C * bands)), dim3(256), lds, as_stream(stream), top_grad,
                       argmax, R, spatial_scale, C, H, W, PH, PW, bottom_grad, rois);
    return launch_status("roi_pool_bwd_kernel");
}

static int roi_align_fwd_impl(const float *features, const float *rois, int R, int B, int C, int H, int W, int AH,
                              int AW, float spatial_scale, float *out, void *stream, int cmajor) {
    if (R < 0 || B <= 0 || C <= 0 || H <= 1 || W <= 1 || AH <= 1 || AW <= 1) { set_error("scda_roi_align_fwd_hip: bad shape"); return SCDA_EINVAL; }
    if ((long long)B * C * H * W > 0x7fffffffLL) { set_error("scda_roi_align_fwd_hip: features exceed int32 indexing"); return SCDA_EINVAL; }
    if (R == 0) return SCDA_OK;
    if (!features || !rois || !out) { set_error("scda_roi_align_fwd_hip: null pointer"); return SCDA_EINVAL; }
    const long long total = (long long)R * C * AH * AW;
    hipLaunchKernelGGL(roi_align_fwd_kernel, dim3(ew_grid(total) * 8), dim3(256), 0, as_stream(stream), total, features,
                       spatial_scale, C, H, W, AH, AW, rois, out, R, cmajor);
    return launch_status("roi_align_fwd_kernel");
}

SCDA_API int scda_roi_align_fwd_hip(const float *features, const float *rois, int R, int B, int C, int H, int W, int AH,
                                    int AW, float spatial_scale, float *out, void *stream) {
    return roi_align_fwd_impl(features, rois, R, B, C, H, W, AH, AW, spatial_scale, out, stream, 0);
}

SCDA_API int scda_roi_align_cmajor_fwd_hip(const float *features, const float *rois, int R, int B, int C, int H, int W, int AH,
                                           int AW, float spatial_scale, float *out, void *stream) {
    return roi_align_fwd_impl(features, rois, R, B, C, H, W, AH, AW, spatial_scale, out, stream, 1);
}

static int roi_align_bwd_impl(const float *top_grad, const float *rois, int R, int B, int C, int H, int W, int AH,
                              int AW, float spatial_scale, float *bottom_grad, void *stream, int cmajor) {
    if (R < 0 || B <= 0 || C <= 0 || H <= 1 || W <= 1 || AH <= 1 || AW <= 1) { set_error("scda_roi_align_bwd_hip: bad shape"); return SCDA_EINVAL; }
    if ((long long)B * C * H * W > 0x7fffffffLL) { set_error("scda_roi_align_bwd_hip: features exceed int32 indexing"); return SCDA_EINVAL; }
    if (R == 0) return SCDA_OK;
    if (!top_grad || !rois || !bottom_grad) { set_error("scda_roi_align_bwd_hip: null pointer"); return SCDA_EINVAL; }
    const long long total = (long long)R * C * AH * AW;
    const size_t lds = (size_t)H * W * sizeof(float);
    // (int)roi[0] * C*H*W must equal the plane the workgroup owns: batch indices are integral in every caller (checked by the
    // reference too, roi_align_kernel.cu:33); planes that do not fit 64 KB of LDS keep the global-atomic form
    if (lds <= 64 * 1024 && AH * AW <= 256 && !getenv("SCDA_ROI_ALIGN_ATOMIC")) {
        hipLaunchKernelGGL(roi_align_bwd_plane_kernel, dim3((unsigned)((long long)B * C)), dim3(256), lds, as_stream(stream), top_grad, R,
                           spatial_scale, C, H, W, AH, AW, bottom_grad, rois, cmajor);
        return launch_status("roi_align_bwd_plane_kernel");
    }
    hipLaunchKernelGGL(roi_align_bwd_kernel, dim3(ew_grid(total) * 8), dim3(256), 0, as_stream(stream), total, top_grad,
                       spatial_scale, C, H, W, AH, AW, bottom_grad, rois, R, cmajor);
    return launch_status("roi_align_bwd_kernel");
}

SCDA_API int scda_roi_align_bwd_hip(const float *top_grad, const float *rois, int R, int B, int C, int H, int W, int AH,
                                    int AW, float spatial_scale, float *bottom_grad, void *stream) {
    return roi_align_bwd_impl(top_grad, rois, R, B, C, H, W, AH, AW, spatial_scale, bottom_grad, stream, 0);
}

SCDA_API int scda_roi_align_cmajor_bwd_hip(const float *top_grad, const float *rois, int R, int B, int C, int H, int W, int AH,
                                           int AW, float spatial_scale, float *bottom_grad, void *stream) {
    return roi_align_bwd_impl(top_grad, rois, R, B, C, H, W, AH, AW, spatial_scale, bottom_grad, stream, 1);
}

#define FOCAL_CHECK(name)                                                             \
    if (N < 0 || num_classes <= 0 || (N % num_classes) != 0) { set_error(name ": bad shape"); return SCDA_EINVAL; } \
    if (N == 0) return SCDA_OK;

SCDA_API int scda_focal_sigmoid_fwd_hip(int N, const float *logits, const int32_t *targets, float weight_pos,
                                        float gamma, float alpha, int num_classes, float *losses, void *stream) {
    FOCAL_CHECK("scda_focal_sigmoid_fwd_hip")
    hipLaunchKernelGGL(focal_sigmoid_fwd_kernel, dim3(ew_grid(N)), dim3(256), 0, as_stream(stream), N, logits, targets,
                       weight_pos, gamma, alpha, num_classes, losses);
    return launch_status("focal_sigmoid_fwd_kernel");
}

SCDA_API int scda_focal_sigmoid_bwd_hip(int N, const float *logits, const int32_t *targets, float *dX,
                                        float weight_pos, float gamma, float alpha, int num_classes, void *stream) {
    FOCAL_CHECK("scda_focal_sigmoid_bwd_hip")
    hipLaunchKernelGGL(focal_sigmoid_bwd_kernel, dim3(ew_grid(N)), dim3(256), 0, as_stream(stream), N, logits, targets,
                       dX, weight_pos, gamma, alpha, num_classes);
    return launch_status("focal_sigmoid_bwd_kernel");
}

SCDA_API int scda_focal_softmax_fwd_hip(int N, const float *logits, const int32_t *targets, float weight_pos,
                                        float gamma, float alpha, int num_classes, float *losses, float *priors,
                                        void *stream) {
    FOCAL_CHECK("scda_focal_softmax_fwd_hip")
    const int rows = N / num_classes;
    hipLaunchKernelGGL(focal_softmax_fwd_kernel, dim3(ew_grid(rows)), dim3(256), 0, as_stream(stream), rows, logits,
                       targets, weight_pos, gamma, alpha, num_classes, losses, priors);
    return launch_status("focal_softmax_fwd_kernel");
}

SCDA_API int scda_focal_softmax_bwd_hip(int N, const float *logits, const int32_t *targets, float *dX,
                                        float weight_pos, float gamma, float alpha, int num_classes,
                                        const float *priors, float *buff, void *stream) {
    (void)logits;
    FOCAL_CHECK("scda_focal_softmax_bwd_hip")
    const int rows = N / num_classes;
    hipLaunchKernelGGL(focal_softmax_bwd_weight_kernel, dim3(ew_grid(rows)), dim3(256), 0, as_stream(stream), rows,
                       priors, targets, buff, weight_pos, gamma, alpha, num_classes);
    int st = launch_status("focal_softmax_bwd_weight_kernel");
    if (st) return st;
    hipLaunchKernelGGL(focal_softmax_bwd_kernel, dim3(ew_grid(N)), dim3(256), 0, as_stream(stream), N, priors, targets,
                       buff, dX, num_classes);
    return launch_status("focal_softmax_bwd_kernel");
}

SCDA_API int scda_iou_overlaps_hip(const float *b1, const float *b2, int size_bbox, int n1, int n2, float *out,
                                   void *stream) {
    if (n1 < 0 || n2 < 0 || size_bbox < 4) { set_error("scda_iou_overlaps_hip: bad shape"); return SCDA_EINVAL; }
    if (n1 == 0 || n2 == 0) return SCDA_OK;
    hipLaunchKernelGGL(iou_overlaps_kernel, dim3(ew_grid((long long)n1 * n2)), dim3(256), 0, as_stream(stream), b1, b2,
                       size_bbox, n1, n2, out);
    return launch_status("iou_overlaps_kernel");
}

SCDA_API int scda_bbox_overlaps_hip(const float *boxes, int N, const float *query, int K, float *out, void *stream) {
    if (N < 0 || K < 0) { set_error("scda_bbox_overlaps_hip: bad shape"); return SCDA_EINVAL; }
    if (N == 0 || K == 0) return SCDA_OK;
    hipLaunchKernelGGL(bbox_overlaps_kernel, dim3(ew_grid((long long)N * K)), dim3(256), 0, as_stream(stream), boxes, N,
                       query, K, out);
    return launch_status("bbox_overlaps_kernel");
}
