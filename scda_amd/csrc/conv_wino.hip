// conv_wino.hip -- Winograd F(2x2, 3x3) convolution on the fp32 MFMA (gfx950): forward and data gradient of the stride-1,
// pad-1 3x3 layers (VGG conv1_2 .. conv5_3, the RPN's 3x3, the decoders' residual convolutions), behind scda_conv2d_wino_hip.
// The reference reaches these layers through cuDNN (nn.Conv2d in models/faster_rcnn/vgg_adver_expansion_cluster.py:101-114,
// models/head.py:13, models/faster_rcnn/common_net.py:59-80), which picks a Winograd algorithm for fp32 3x3 itself.
//
//   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A         per 2x2 output tile, 4x4 input tile d, 3x3 filter g
// 16 transform-domain positions xi = (a, b); per position a plain GEMM  M_xi[m][t] = sum_c U_xi[m][c] V_xi[c][t]  over tiles t:
// 16 multiplies per 4 outputs instead of 36 -- 2.25x fewer MFMA operations than the direct implicit GEMM of conv_gemm.hip,
// whose K loop already runs at the matrix pipe's sustained rate.
//
// One workgroup = 64 output channels x 64 tiles (4 tile rows x 16 tile columns = 8 x 32 output pixels of one image), all 16
// positions, 8 waves.  Wave w owns TWO positions, xi = (a = w >> 1, b in {1, 2} or {0, 3}), and for them the whole 64 x 64
// accumulator block (2 x 2 x 2 MFMA tiles = 128 accumulator registers).  Consequences:
//   * U (the transformed weights) is needed by ONE wave only -> it never goes through LDS: scda_conv2d_pack_* lays it out in
//     the MFMA A-fragment order, one global_load_dwordx4 per (position, 32-row block, 8-channel slab) and lane, prefetched one
//     slab ahead into registers.  The m-tile is the fastest grid dimension, so XCD x mostly serves m-tile x % n_mt and its
//     16 x 64 x C weights stay in that XCD's L2.
//   * V is never materialised.  BT has two non-zeros per row, so V_ab[c][t] is a signed sum of FOUR raw input values; LDS holds
//     only the raw (8 + 2) x (32 + 2) input patch of the slab's 8 channels (12.8 KB per stage, LDS-DMA, ring of 4), and every
//     wave forms its own B fragments with 4 ds_read_b32 + 4 VALU per pair of positions (b in {1, 2} share their reads) or 8 + 6
//     (b in {0, 3}).  Even and odd patch columns are stored apart (lane offsets chosen by the LDS-DMA's per-lane source address),
//     so a half-wave's 32 tiles read 32 consecutive banks.
//   * every wave also issues a share of the patch LDS-DMA (7 dword instructions per slab): dedicated staging waves would make it
//     10 waves = 3 on some SIMDs = 168 registers per lane, less than the 128 accumulators + fragments need.
// Ordering: vmcnt is in-order, a wave issues per slab [patch DMA for slab s+2][U loads for slab s+1] and waits for its U(s) before
// the MFMAs of slab s -- which implies its DMA(s+1) has landed before barrier s+1.  One s_barrier per slab.
// Epilogue: the 16 positions of an output tile live in 8 different waves: exchanged through LDS (32 rows at a time, 128 KB), then
// every thread applies A^T . A to its (channel, tile) pairs and stores 2 x 2 pixels (+ bias, activation, the producer's act' mask
// -- or a split-K slab in the natural pixel order, combined by conv_gemm.hip's reduce kernel).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "launch_plan.h"
#include "mfma_tile.h"
#include "wino_pack.h"

namespace scda {

int launch_conv_reduce(const float *ws, int splits, int M, int N, int phw, const float *bias, int act, float slope, float *out,
                       const float *mask_src, float mask_slope, hipStream_t st);   // conv_gemm.hip
int launch_wgrad_reduce(const float *ws, int splits, long long total, int N, int accumulate, float *out, const float *db_ws, float *db,
                        int db_n, int db_accumulate, hipStream_t st);               // conv_gemm.hip

typedef __attribute__((address_space(3))) void wino_lds_void_t;
#if defined(__HIP_DEVICE_COMPILE__)
// LDS-DMA through a buffer descriptor over [base, base + 2 GB): a lane offset with bit 31 set lands as 0.0 (see conv_gemm.hip)
__device__ __forceinline__ void wino_dma_b32(const void *base, const unsigned voffset, float *lds_dst, const int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(__builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)0x80000000u, 0x00020000),
                                             (wino_lds_void_t *)lds_dst, 4, voffset, soffset, 0, 0);
}
#else
__device__ __forceinline__ void wino_dma_b32(const void *, const unsigned, float *, const int) {}
#endif
#ifndef SCDA_WINO_ABLATE
#define SCDA_WINO_ABLATE 0     // timing ablations of conv_wino_kernel's K loop (scripts/ablate/wino_ablate.sh): 4 no barrier, 8 no patch DMA, 16 no LDS reads; weight gradient: 128 / 64 / 32, 256 no epilogue, 512 no operand transforms, 1024 epilogue without its stores
#endif
#define WINO_WAIT_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
// An empty volatile asm that "rewrites" a register value: it is ordered among the side-effecting nodes (sched_barrier, s_barrier, the
// other pins), so a PURE operation -- an MFMA, a VALU sum: nodes without a chain, which instruction selection is free to bunch up
// across sched_barriers, and did in the {0, 3} column variant -- whose operand is pinned in front of it and whose result is pinned
// behind it stays in the slot it was written in.  No instruction is emitted.
#define WINO_PIN(x) asm volatile("" : "+v"(x))
// LDS hand-over inside a workgroup WITHOUT draining the vector-memory counter: __syncthreads() is fence + barrier, and the fence
// waits vmcnt(0) -- for the persistent kernel's epilogue that is the next tile's patch requests and the previous passes' stores
#define WINO_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

constexpr int WBK = WINO_BK;                    // channels per K-slab (8)
constexpr int W_PR = 10, W_RS = 40;             // patch rows; row stride in floats: 17 even columns at 0.., 17 odd columns at 20..
constexpr int W_CS = W_PR * W_RS;               // channel stride
constexpr int W_DMA = 7;                        // LDS-DMA instructions per wave and slab: 8 x 7 x 64 slots >= 8 channels x 400
constexpr int W_STAGE = 8 * W_DMA * 64;         // floats per ring stage (3584)
constexpr int W_NST = 4;
constexpr int W_MX = 16 * 16 * 64;              // epilogue exchange per 16 rows: [position][rows][64 tiles]
static_assert(W_NST * W_STAGE <= W_MX && WBK * W_CS <= W_STAGE, "the ring lives inside the exchange buffer");

struct WinoGeom {
    int batch, C, H, W, M;
    int n_mt, n_mbg, n_slab, slabs_per_split;   // m-tiles of the launch (32 * MB rows each); 32-row blocks of the packed filters
    Div dNMT, dNPB, dNB, dNBX;   // m-tiles; pixel blocks of the launch; per image; per block row
    int pixel_major, npb, per_xcd;   // XCD-aware order with the pixel block outermost (see the kernel); pixel blocks of the launch;
                                     // (split, pixel block) items per XCD
    int n_wg;                        // tiles (workgroup slots) of the launch: what a one-tile-per-workgroup grid would be
    int stack;                       // > 0: the image [1, C, stack * 7, 7] is a vertical stack of that many independent 7 x 7 maps (row
                                     // period 7: the channel-major RoI head of the ResNet-50 C4 detector).  A pixel block = FOUR maps side
                                     // by side as 8 x 8 each (4 x 4 tiles, row / column 7 discarded): in patch coordinates a map's columns
                                     // sit at 8 k + 1 .. 8 k + 7 with ONE zero column between neighbours -- it is the left padding of map
                                     // k and the (non-existent) column 7 of map k - 1 at once -- and rows 1 .. 7 between two zero rows, so
                                     // the K loop is the plain one; only the patch offsets and the output addressing differ
    int gm_mask, gm_shift;           // ... with the 8 XCDs split gm x (8 / gm) over m-tile groups x pixel-block runs: gm - 1, log2(gm)
    Div dNML;                        // m-tiles per XCD (n_mt / gm)
};

struct WinoEpi {
    float *out, *ws;
    const float *bias;
    int act;
    float slope;
    int splits;
    const float *mask_src;
    float mask_slope;
    int dbg;   // ablation knob (SCDA_WINO_DBG): 1 = no epilogue, 2 = no K loop
    float *pool_y;          // non-null: FUSED 2x2 max-pool -- the tile's four outputs are one pooling window; only the pooled value
    unsigned char *pool_idx;   // [batch, M, H/2, W/2] and the winner 0..3 are stored (scda_maxpool2x2_fwd_hip's conventions), not the map
};

typedef float wino_f4 __attribute__((ext_vector_type(4)));
typedef float wino_f2 __attribute__((ext_vector_type(2)));

// MB = 32-row blocks of output channels per workgroup.  2: 64 x 64 tile, 128 accumulator registers per wave -- one workgroup per
// CU; every U and V fragment feeds two MFMAs.  1: 32 x 64 tile, 64 accumulators, 64 KB of LDS -- TWO workgroups per CU (4 waves per
// SIMD at <= 128 registers): for layers with <= 32 output rows and launches that would not fill the chip with 64-row tiles.
//
// PERSIST (MB = 2, launches of more tiles than CUs): one workgroup per CU walks tiles b = blockIdx.x, + gridDim.x, ... (gridDim.x a
// multiple of 8: the XCD a tile runs on, and with it the launch orders below, are those of the one-tile-per-workgroup launch).  What
// a tile costs outside its K loop -- 6 us of start-up (workgroup dispatch, first patch + U round trip) and 6 us of epilogue on top
// of conv1_2's 17 us of K loop, with all workgroups of a round storing at the same time -- is taken apart:
//   * the exchange buffer is 16 rows per pass (64 KB, four passes) and the ring lies BEHIND it, so the next tile's first three
//     patches and its first U fragments are requested before the current tile's epilogue and have landed when it ends;
//   * the epilogue's stores are unconditional buffer stores (tiles / rows outside the tensor get an offset the descriptor's range
//     check drops) and nothing waits for them by name: they drain underneath the next tile's K loop.  The counted waits of that K
//     loop count LOADS only (patch LDS-DMA and U fragments, which retire in issue order); a first version added the epilogue's 16
//     stores to the counts of the next tile's first two hand-overs (stores being younger than the patches they wait for) and was
//     wrong one launch in a few hundred -- a replayed-graph iteration differed from the eager one in the last bits to the third
//     digit: on gfx950 store acknowledgements (and certainly range-dropped stores) do NOT retire in issue order with older LDS-DMA
//     loads, so "at most N outstanding" says nothing about a load once stores are among the N.  With loads-only counts a wait is
//     at worst early-satisfied by nothing and at best released by stores retiring early; either way the patch it names has landed.

#if defined(__HIP_DEVICE_COMPILE__)
typedef int wino_i2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wino_rsrc(const void *base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)0x80000000u, 0x00020000);
}
#endif

// EPI: what the epilogue does with a finished 2 x 2 output tile, a compile-time choice so that every variant is straight-line code
// with a known number of vector-memory instructions (the compiler's counted waits are the minimum over the paths it sees):
// 0 bias + activation, 1 + the producer's activation mask (data gradient), 2 + fused 2x2 max-pool, 3 a split-K slab
enum { WEPI_PLAIN = 0, WEPI_MASK = 1, WEPI_POOL = 2, WEPI_SPLIT = 3 };

template <int MB, bool PERSIST, int EPI>
__global__ __launch_bounds__(512, (MB == 2 ? 2 : 4)) void conv_wino_kernel(const float *__restrict__ U, const float *__restrict__ X,
                                                                        const WinoGeom g, const WinoEpi e) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(!PERSIST || MB == 2, "the persistent form is the one-workgroup-per-CU tile");
    constexpr int RP = PERSIST ? 16 : 16 * MB;         // output-channel rows per exchange pass
    constexpr int NPASS = 32 * MB / RP;
    constexpr int NRG = RP / 2;                        // accumulator registers per tile and pass
    constexpr int XCH = 16 * RP * 64;                  // exchange buffer (floats): [position][row][64 tiles]
    constexpr int RING = PERSIST ? XCH : 0;            // first float of the ring: behind the exchange buffer, or aliasing it
    static_assert(PERSIST || W_NST * W_STAGE <= XCH, "the ring lives inside the exchange buffer");
    constexpr int BIAS = PERSIST ? XCH + W_NST * W_STAGE : XCH;     // 2 x 64 floats behind everything: the bias values of this tile and of the next
    __shared__ __attribute__((aligned(16))) float lds[BIAS + 128];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int plane = g.H * g.W;
    const int N = g.batch * plane;

    // ---- tile b of the launch -> (m-tile, split, image, pixel block); false: an idle slot of an XCD's run ---------------------------
    struct Tile { int mt, sp, img, y0, x0, s_begin, s_end; };
    auto decode = [&](const int b, Tile &t) -> bool {
        int rest, pb, bi, by, bx;
        if (g.pixel_major) {
            // workgroup b runs on XCD b % 8.  Inside an XCD's sequence the m-tile is fastest and a pixel block's m-tiles are consecutive:
            // one XCD's L2 fetches a patch once for all of them (m-tile-major puts the m-tiles of a block on DIFFERENT XCDs: the input
            // crosses the fabric n_mt times); the XCD then needs every m-tile's filters, which is why the launcher only picks this order
            // when all 16 x M x C of them fit an L2.  An XCD owns a CONTIGUOUS run of (split, pixel block) items -- row neighbours run side
            // by side on it and share the 128-byte lines their 136-byte patch rows straddle (the halo columns make every row touch three
            // lines: dealt round-robin, neighbouring blocks landed on different XCDs and each fetched the shared lines itself).
            // With the filters too large for that (conv4_x: 8 - 17 MB) the XCDs are split gm x (8 / gm): XCD x serves the m-tiles
            // mt % gm == x % gm on run x / gm of the pixel blocks -- each XCD streams 1 / gm of the filters and reads 1 / (8 / gm) of
            // the input, instead of one m-tile's filters and the WHOLE input (m-tile-major).
            const int x = b & 7, j = b >> 3;
            int pl, ml;
            g.dNML.divmod(j, pl, ml);
            t.mt = (ml << g.gm_shift) + (x & g.gm_mask);
            rest = (x >> g.gm_shift) * g.per_xcd + pl;
            if (pl >= g.per_xcd || rest >= g.npb * e.splits) return false;
            g.dNPB.divmod(rest, t.sp, pb);
        } else {
            g.dNMT.divmod(b, rest, t.mt);
            g.dNPB.divmod(rest, t.sp, pb);
        }
        g.dNB.divmod(pb, t.img, bi);
        g.dNBX.divmod(bi, by, bx);
        t.y0 = by * 8; t.x0 = bx * 32;
        t.s_begin = t.sp * g.slabs_per_split; t.s_end = min(g.n_slab, t.s_begin + g.slabs_per_split);
        return true;
    };
    auto next_tile = [&](int &b, Tile &t) -> bool {     // the next tile of this workgroup behind b, if any
        if (!PERSIST) return false;
        for (b += (int)gridDim.x; b < g.n_wg; b += (int)gridDim.x)
            if (decode(b, t)) return true;
        return false;
    };

    // ---- this wave's two positions ------------------------------------------------------------------------------------------------
    // waves w and w + 4 share a SIMD (a workgroup's waves go to the SIMDs cyclically): one of each column set per SIMD -- the {0, 3} waves
    // read and add twice as much per fragment as the {1, 2} waves, and every slab ends in a barrier
    const int a = wave & 3, bsel = wave >> 2;
    const int xi0 = a * 4 + (bsel ? 1 : 0), xi1 = a * 4 + (bsel ? 2 : 3);
    // BT row a = signed sum of patch rows i1, i2:  0: d0 - d2   1: d1 + d2   2: d2 - d1   3: d1 - d3
    const int i1 = a == 0 ? 0 : a == 2 ? 2 : 1, i2 = a == 0 ? 2 : a == 1 ? 2 : a == 2 ? 1 : 3;
    const float sgn = a == 1 ? 1.f : -1.f;
    const int j = lane & 31, h = lane >> 5;
    const int lane_base = RING + h * W_CS + (2 * (j >> 4)) * W_RS + (j & 15);
    const int ro1 = lane_base + i1 * W_RS, ro2 = lane_base + i2 * W_RS;
    const int n_mbg = g.n_mbg;

    // ---- what the K loop needs of a tile: patch offsets, image base, U bases, slab range -----------------------------------------------
    struct Ctx {
        unsigned dma_off[W_DMA];
        const char *xbase;
        unsigned uoff[2][MB];        // U fragments: wave-uniform byte offset per (position, 32-row block); + lane * 16; one slab = 1 KB further on
        int s_begin, s_end;
    };
    auto setup = [&](const Tile &t, Ctx &c) {
        // this wave's share of the patch LDS-DMA: slot -> (channel, patch row, column) is fixed, the tile moves the patch (recomputed
        // per tile: ~70 VALU against seven registers held across the K loop)
        int ln = lane;
        WINO_PIN(ln);       // (opaque per call: hoisted out of the tile loop, the seven decompositions were SPILLED across it)
#pragma unroll
        for (int i = 0; i < W_DMA; ++i) {
            const int slot = (wave * W_DMA + i) * 64 + ln;
            const int ch = slot / W_CS, rem = slot - ch * W_CS;
            const int row = rem / W_RS, sl = rem - row * W_RS;
            const int col = sl < 17 ? 2 * sl : (sl >= 20 && sl < 37) ? 2 * (sl - 20) + 1 : -1;
            if (g.stack) {      // patch column col >= 1: map (col - 1) / 8 of the block's four, its column (col - 1) % 8; row - 1 = its row
                const int map = (t.y0 >> 1) + ((col - 1) >> 3), mx = (col - 1) & 7, my = row - 1;
                const bool ok = ch < WBK && col >= 1 && col <= 32 && mx < 7 && (unsigned)my < 7u && map < g.stack;
                c.dma_off[i] = ok ? (unsigned)((ch * plane + (map * 7 + my) * 7 + mx) * 4) : 0x80000000u;
                continue;
            }
            const int gy = t.y0 - 1 + row, gx = t.x0 - 1 + col;
            const bool ok = ch < WBK && col >= 0 && (unsigned)gy < (unsigned)g.H && (unsigned)gx < (unsigned)g.W;
            c.dma_off[i] = ok ? (unsigned)((ch * plane + gy * g.W + gx) * 4) : 0x80000000u;
        }
        c.xbase = reinterpret_cast<const char *>(X + (size_t)t.img * g.C * plane);
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
                c.uoff[x][mb] = (unsigned)(((x ? xi1 : xi0) * n_mbg + t.mt * MB + mb) * g.n_slab) * 1024u;
        c.s_begin = t.s_begin; c.s_end = t.s_end;
    };
    auto issue_dma_one = [&](const Ctx &c, const int s, const int buf, const int i) {
        wino_dma_b32(c.xbase, c.dma_off[i], lds + RING + buf * W_STAGE + wave * (W_DMA * 64) + i * 64, s * (WBK * plane * 4));
    };
    auto issue_dma = [&](const Ctx &c, const int s, const int buf) {
#pragma unroll
        for (int i = 0; i < W_DMA; ++i) issue_dma_one(c, s, buf, i);
    };
    // (a buffer load: descriptor + scalar offset + one lane offset shared by all of them -- as global loads the compiler kept a 64-bit
    // lane address per (position, block) in registers across the loop and added the slab offset on the vector unit)
    const __amdgpu_buffer_rsrc_t r_u = wino_rsrc(U);
    auto load_a_one = [&](const Ctx &c, const int s, const int x, const int mb, wino_f4 (&A)[2][MB]) {
#if defined(WINO_DBG_U_GLOBAL)
        A[x][mb] = *reinterpret_cast<const wino_f4 *>(reinterpret_cast<const char *>(U) + c.uoff[x][mb] + (size_t)s * 1024 + lane * 16);
        return;
#endif
        A[x][mb] = __builtin_bit_cast(wino_f4, __builtin_amdgcn_raw_buffer_load_b128(r_u, lane * 16, (int)(c.uoff[x][mb] + (unsigned)s * 1024u), 0));
    };

    f32x16 acc[2][MB][2];
    wino_f4 A0[2][MB], A1[2][MB];
    // a tile's first requests: patches of its first three slabs into ring stages 0 - 2, the U fragments of its first slab.  VMEM order
    // = the steady state's (patch, patch, U, patch): the compiler's counted waits for the U fragments at the loop head are the
    // minimum over the ways into it
    // (the bias goes the same way, as the OLDEST request: 64 rows = one LDS-DMA instruction, issued by every wave alike -- the counted
    // waits below count per wave.  Not a scalar load: the scalar cache kept last iteration's values inside a replayed hipGraph; not
    // a vector load in the epilogue: its result could only be waited for together with every older request and store)
    auto first_requests = [&](const Ctx &c, const Tile &t, const int par) {
        if (EPI != WEPI_SPLIT) {
            const int m = t.mt * (32 * MB) + lane;
            wino_dma_b32(e.bias, (e.bias && lane < 32 * MB && m < g.M) ? (unsigned)(m * 4) : 0x80000000u, lds + BIAS + 64 * par, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        issue_dma(c, c.s_begin, 0);
        __builtin_amdgcn_sched_barrier(0);
        issue_dma(c, min(c.s_begin + 1, c.s_end - 1), 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) load_a_one(c, c.s_begin, x, mb, A0);
        __builtin_amdgcn_sched_barrier(0);
        issue_dma(c, min(c.s_begin + 2, c.s_end - 1), 2);
        __builtin_amdgcn_sched_barrier(0);
    };

    // the K loop, compiled once per column set (BSEL: b in {1, 2} -- four raw values per fragment pair -- or {0, 3} -- eight).
    // A software pipeline over K-PAIRS (one K-pair = 2 channels = one MFMA per accumulator block), written slot by slot and pinned
    // with sched_barriers: left to itself the scheduler sinks every ds_read next to its use and waits lgkmcnt(0) behind it, and
    // issues the slab's 7 LDS-DMA + 2 MB U loads as one burst behind the barrier -- both waves of a SIMD then sit in the same
    // LDS / issue latency at the same time and the matrix pipe idles (54 % busy, 62 % of the waves' cycles stalled at issue).
    //   step i (K-pair i):  slot m = [MFMA m of K-pair i][a share of: VALU of K-pair i + 1, ds_reads of K-pair i + 2, one VMEM]
    // A tile block's raw values are consumed (BT-row sums) in the first half of a step and re-read for the K-pair after next behind
    // that, so a raw value is read 3 MB MFMAs (>= 192 cycles) before the VALU that consumes it, in the same registers, and a B
    // fragment is formed one step before its MFMAs; the U loads of slab s + 1 ride in steps 0 - 1, the patch DMA of slab s + 3 in
    // steps 2 - 3.  The hand-over (counted vmcnt + s_barrier) for slab s + 1 sits in the MIDDLE of slab s's MFMA stream, behind the
    // first MFMA of step 2: the first reads of the next patch are issued there, a step and a half before they are needed.
    auto k_loop = [&](auto bsel_tag, const Ctx &c) {
        constexpr bool BSEL = decltype(bsel_tag)::value;
        constexpr int NR = BSEL ? 4 : 8;          // raw values per tile block and K-pair
        constexpr int NSLOT = 4 * MB;             // MFMAs per K-pair
        const int s_end = c.s_end;
        float raw[2][NR];                         // [tile block][value]: K-pair i + 1 until its sums are formed, then K-pair i + 2
        float pt[2][4];                           // BT-row sums of the K-pair being formed
        float v[2][2][2];                         // [ring of 2 K-pairs][position][tile block]
        auto read_unit = [&](const float *st, const int kp, const int tb, const int q) {
#if (SCDA_WINO_ABLATE & 16)
            raw[tb][q] = sgn;                     // ablation: no LDS reads
            return;
#endif
            const float *r = st + ((q >= NR / 2) ? ro2 : ro1) + 2 * kp * W_CS + tb * 4 * W_RS;
            // patch columns: BSEL 1, 2 -- slots 20, 1;  otherwise 0, 2, 1, 3 -- slots 0, 1, 20, 21 (odd columns live at 20..)
            const int qq = q % (NR / 2);
            raw[tb][q] = r[BSEL ? (qq ? 1 : 20) : (qq == 0 ? 0 : qq == 1 ? 1 : qq == 2 ? 20 : 21)];
        };
        auto valu_a = [&](const int tb) {         // BT row a over the two patch rows
#pragma unroll
            for (int q = 0; q < NR / 2; ++q) {
                WINO_PIN(raw[tb][q]);
                pt[tb][q] = raw[tb][q] + sgn * raw[tb][q + NR / 2];
                WINO_PIN(pt[tb][q]);
            }
        };
        auto valu_b = [&](const int tb, float (&V)[2][2]) {
            if (BSEL) {
                V[0][tb] = pt[tb][0] + pt[tb][1];        // b = 1: d1 + d2
                V[1][tb] = pt[tb][1] - pt[tb][0];        // b = 2: d2 - d1
            } else {
                V[0][tb] = pt[tb][0] - pt[tb][1];        // b = 0: d0 - d2
                V[1][tb] = pt[tb][2] - pt[tb][3];        // b = 3: d1 - d3
            }
            WINO_PIN(V[0][tb]);
            WINO_PIN(V[1][tb]);
        };
        // one step = the MFMAs of K-pair kp of the slab in ring stage `buf`
        auto step = [&](const int kp, const int s, const int buf, wino_f4 (&Acur)[2][MB], wino_f4 (&Anext)[2][MB]) {
            const float *rst = lds + ((buf + (kp >= 2 ? 1 : 0)) & (W_NST - 1)) * W_STAGE;
            const int rkp = (kp + 2) & 3, rb = kp & 1;
#pragma unroll
            for (int m = 0; m < NSLOT; ++m) {
                const int x = m / (2 * MB), mb = (m / 2) % MB, tb = m & 1;
                WINO_PIN(v[rb][x][tb]);
                acc[x][mb][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Acur[x][mb][kp], v[rb][x][tb], acc[x][mb][tb], 0, 0, 0);
                WINO_PIN(acc[x][mb][tb]);
                if (kp == 2 && m == 0) {
                    // hand-over for the NEXT slab behind an MFMA: this wave's share of its patch has landed -- younger than it are only
                    // the U loads of two slabs and one slab's DMA
                    __builtin_amdgcn_sched_barrier(0);
                    WINO_WAIT_VMCNT(W_DMA + 4 * MB);
#if !(SCDA_WINO_ABLATE & 4)
                    __builtin_amdgcn_s_barrier();
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
                // quarter h of the step: sums of tile block h >> 1 (h even), its fragments + its re-read (h odd)
                const int h4 = m / MB, sub = m % MB;
                if ((h4 & 1) == 0) {
                    if (sub == MB - 1) valu_a(h4 >> 1);
                } else {
#pragma unroll
                    for (int q = sub * (NR / MB); q < (sub + 1) * (NR / MB); ++q) read_unit(rst, rkp, h4 >> 1, q);
                    if (sub == MB - 1) valu_b(h4 >> 1, v[rb ^ 1]);
                }
                // VMEM, issued UNCONDITIONALLY with clamped slab indices (behind a branch the compiler's waitcnt pass must assume the
                // loads were not issued and drains the prefetch with vmcnt(0); the clamped tail loads go to a stage / registers nobody reads)
                if (kp < 2) {
                    const int um = (m == 0) ? 0 : (MB == 2 && m == 4) ? 1 : -1;
                    if (um >= 0) load_a_one(c, min(s + 1, s_end - 1), kp, um, Anext);
                } else {
#if !(SCDA_WINO_ABLATE & 8)
                    const int di = MB == 2 ? ((m & 1) ? -1 : (kp - 2) * 4 + (m >> 1)) : (kp - 2) * 4 + m;
                    if (di >= 0 && di < W_DMA) issue_dma_one(c, min(s + 3, s_end - 1), (buf + 3) & (W_NST - 1), di);
#endif
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto slab = [&](const int s, const int buf, wino_f4 (&Acur)[2][MB], wino_f4 (&Anext)[2][MB]) {
#pragma unroll
            for (int kp = 0; kp < WBK / 2; ++kp) step(kp, s, buf, Acur, Anext);
        };
        // the first patch has landed (this wave's share: younger LOADS are two patches and the U fragments)
        WINO_WAIT_VMCNT(2 * W_DMA + 2 * MB);
        __builtin_amdgcn_s_barrier();
        {   // fill the pipeline: B fragments of K-pair 0, raw values of K-pair 1
            const float *st0 = lds;
#pragma unroll
            for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                for (int q = 0; q < NR; ++q) read_unit(st0, 0, tb, q);
#pragma unroll
            for (int tb = 0; tb < 2; ++tb) { valu_a(tb); valu_b(tb, v[0]); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                for (int q = 0; q < NR; ++q) read_unit(st0, 1, tb, q);
            __builtin_amdgcn_sched_barrier(0);
        }
        int s = c.s_begin, buf = 0;
        for (; s + 1 < s_end; s += 2) {
            slab(s, buf, A0, A1);
            slab(s + 1, (buf + 1) & (W_NST - 1), A1, A0);
            buf = (buf + 2) & (W_NST - 1);
        }
        if (s < s_end) slab(s, buf, A0, A1);
        if (!PERSIST) WINO_WAIT_VMCNT(0);      // the clamped tail DMA must not land in the exchange buffer below (PERSIST: the ring is its own)
    };

    // ---- epilogue: exchange the 16 positions through LDS, output transform, store ---------------------------------------------------
    // NPASS passes of RP output-channel rows: accumulator registers r with frag_row(r) = (r & 3) + 8 * (r >> 2) + 4 * h in the pass's
    // rows.  Stores are buffer stores with the range check as the guard (no branch around a memory instruction: a wave issues the same
    // stores for every tile).
    auto epilogue = [&](const Tile &t, const int par) {
        // (lane-derived constants of the epilogue are re-derived per tile from an opaque copy of the lane id: hoisted out of the tile
        // loop they would be live across the K loop, which has no register to spare)
        int ln = lane;
        WINO_PIN(ln);
        const int j = ln & 31, h = ln >> 5;
        const __amdgpu_buffer_rsrc_t r_out = wino_rsrc(EPI == WEPI_SPLIT ? (const void *)(e.ws + (size_t)t.sp * g.M * N + (size_t)t.img * plane)
                                                       : EPI == WEPI_POOL ? (const void *)(e.pool_y + (size_t)t.img * g.M * (plane >> 2))
                                                                          : (const void *)(e.out + (size_t)t.img * g.M * plane));
        const __amdgpu_buffer_rsrc_t r_idx = wino_rsrc(EPI == WEPI_POOL ? (const void *)(e.pool_idx + (size_t)t.img * g.M * (plane >> 2)) : (const void *)e.out);
        const __amdgpu_buffer_rsrc_t r_msk = wino_rsrc(EPI == WEPI_MASK ? (const void *)(e.mask_src + (size_t)t.img * g.M * plane) : (const void *)e.out);
        // stacked 7 x 7 maps: tile column tc of the block belongs to map tc >> 2; the tile's pixels (row 2 tr + a, column 2 (tc & 3) + b)
        // exist where the coordinate is < 7 -- four single stores with their own range checks instead of two pairs
        const int s_map = (t.y0 >> 1) + ((ln & 15) >> 2), s_y = 2 * (ln >> 4), s_x = 2 * (ln & 3);
        const int oy = g.stack ? s_map * 7 + s_y : t.y0 + 2 * (ln >> 4), ox = g.stack ? s_x : t.x0 + 2 * (ln & 15);
        const bool in_img = g.stack ? s_map < g.stack : (oy < g.H && ox < g.W);      // (H, W even: a tile is inside the image or outside, never across)
        const bool s_row1 = s_y + 1 < 7, s_col1 = s_x + 1 < 7;
        const unsigned pix = (unsigned)(oy * g.W + ox);
        auto out_off = [&](const int pass, const int q) -> unsigned {     // byte offset of (row m, this lane's tile) in the full-resolution map
            const int m = t.mt * (32 * MB) + pass * RP + q * 8 + wave;
            return (in_img && m < g.M) ? (unsigned)(((size_t)m * plane + pix) * 4) : 0x80000000u;
        };
        // the producer's activation mask of the data gradient: loaded ONE PASS AHEAD, so that waiting for it does not wait for this
        // pass's stores
        wino_f2 mk[RP / 8][2];
        auto stack_off = [&](const unsigned o, const int k) -> unsigned {      // element k = 2 a + b of a stacked map's tile
            const bool ok = o != 0x80000000u && (!(k & 1) || s_col1) && (!(k >> 1) || s_row1);
            return ok ? o + (unsigned)(((k >> 1) * 7 + (k & 1)) * 4) : 0x80000000u;
        };
        auto load_mask = [&](const int pass) {
#pragma unroll
            for (int q = 0; q < RP / 8; ++q) {
                const unsigned o = out_off(pass, q);
                if (g.stack) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        mk[q][k >> 1][k & 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_msk, stack_off(o, k), 0, 0));
                    continue;
                }
                mk[q][0] = __builtin_bit_cast(wino_f2, __builtin_amdgcn_raw_buffer_load_b64(r_msk, o, 0, 0));
                mk[q][1] = __builtin_bit_cast(wino_f2, __builtin_amdgcn_raw_buffer_load_b64(r_msk, o, g.W * 4, 0));
            }
        };
        auto store4 = [&](const __amdgpu_buffer_rsrc_t r, const unsigned o, const float a, const float b2, const float c2, const float d) {
            if (g.stack) {
                const float v[4] = {a, b2, c2, d};
#pragma unroll
                for (int k = 0; k < 4; ++k) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v[k]), r, stack_off(o, k), 0, 0);
                return;
            }
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wino_i2, wino_f2{a, b2}), r, o, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wino_i2, wino_f2{c2, d}), r, o, g.W * 4, 0);
        };
        constexpr bool masked = EPI == WEPI_MASK;
        if (masked) load_mask(0);
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            const int mb = pass * RP / 32, r0 = (pass * RP % 32) / 2;      // 32-row block; first accumulator register of the pass
            WINO_LDS_BARRIER();    // the ring (first pass, non-persistent) / the previous pass's reads are done
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                float *mx = lds + (x ? xi1 : xi0) * (RP * 64) + j;
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                    for (int rr = 0; rr < NRG; ++rr) {
                        const int r = r0 + rr;
                        const int row = ((r & 3) + 8 * (r >> 2) + 4 * h) - (pass * RP % 32);
                        mx[row * 64 + tb * 32] = acc[x][mb][tb][r];
                    }
            }
            WINO_LDS_BARRIER();
            float y[RP / 8][4];
#pragma unroll
            for (int q = 0; q < RP / 8; ++q) {
                const float *mp = lds + (q * 8 + wave) * 64 + ln;
                float t0[4], t1[4];
#pragma unroll
                for (int aa = 0; aa < 4; ++aa) {
                    const float m0 = mp[(aa * 4 + 0) * (RP * 64)], m1 = mp[(aa * 4 + 1) * (RP * 64)], m2 = mp[(aa * 4 + 2) * (RP * 64)], m3 = mp[(aa * 4 + 3) * (RP * 64)];
                    t0[aa] = m0 + m1 + m2;
                    t1[aa] = m1 - m2 - m3;
                }
                y[q][0] = t0[0] + t0[1] + t0[2]; y[q][1] = t1[0] + t1[1] + t1[2];
                y[q][2] = t0[1] - t0[2] - t0[3]; y[q][3] = t1[1] - t1[2] - t1[3];
            }
            wino_f2 mcur[RP / 8][2];
            if (masked) {
#pragma unroll
                for (int q = 0; q < RP / 8; ++q) { mcur[q][0] = mk[q][0]; mcur[q][1] = mk[q][1]; }
                if (pass + 1 < NPASS) load_mask(pass + 1);
            }
#pragma unroll
            for (int q = 0; q < RP / 8; ++q) {
                const int m = t.mt * (32 * MB) + pass * RP + q * 8 + wave;
                float y00 = y[q][0], y01 = y[q][1], y10 = y[q][2], y11 = y[q][3];
                const unsigned o = out_off(pass, q);
                if (EPI == WEPI_SPLIT) {      // a split-K slab in the natural pixel order: ws[split][m][image][pixel]
                    const unsigned os = (in_img && m < g.M) ? (unsigned)(((size_t)m * N + pix) * 4) : 0x80000000u;
                    store4(r_out, os, y00, y01, y10, y11);
                    continue;
                }
#if defined(WINO_DBG_BIAS_VEC)
                if (e.bias) { const float bv = e.bias[min(m, g.M - 1)]; y00 += bv; y01 += bv; y10 += bv; y11 += bv; }
#else
                if (e.bias) { const float bv = lds[BIAS + 64 * par + pass * RP + q * 8 + wave]; y00 += bv; y01 += bv; y10 += bv; y11 += bv; }
#endif
                y00 = apply_act(y00, e.act, e.slope); y01 = apply_act(y01, e.act, e.slope);
                y10 = apply_act(y10, e.act, e.slope); y11 = apply_act(y11, e.act, e.slope);
                if (EPI == WEPI_POOL) {      // the window's winner: first maximum in (0,0) (0,1) (1,0) (1,1) order, NaN wins (maxpool2_fwd_kernel)
                    float mv = y00;
                    int kk = 0;
                    if (y01 > mv || y01 != y01) { mv = y01; kk = 1; }
                    if (y10 > mv || y10 != y10) { mv = y10; kk = 2; }
                    if (y11 > mv || y11 != y11) { mv = y11; kk = 3; }
                    const unsigned po = (unsigned)((size_t)m * (plane >> 2) + (size_t)(oy >> 1) * (g.W >> 1) + (ox >> 1));
                    const bool ok = in_img && m < g.M;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, mv), r_out, ok ? po * 4u : 0x80000000u, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)kk, r_idx, ok ? po : 0x80000000u, 0, 0);
                    continue;
                }
                if (masked) {
                    const wino_f2 k0 = mcur[q][0], k1 = mcur[q][1];
                    y00 = k0[0] > 0.f ? y00 : y00 * e.mask_slope; y01 = k0[1] > 0.f ? y01 : y01 * e.mask_slope;
                    y10 = k1[0] > 0.f ? y10 : y10 * e.mask_slope; y11 = k1[1] > 0.f ? y11 : y11 * e.mask_slope;
                }
                store4(r_out, o, y00, y01, y10, y11);
            }
        }
    };

    // ---- the tile loop ---------------------------------------------------------------------------------------------------------------
    Tile tile, tnext;
    Ctx cur;
    int b = (int)blockIdx.x;
    bool have = decode(b, tile);
    if (!have) have = next_tile(b, tile);
    if (!have) return;
    setup(tile, cur);
    int par = 0;        // which of the two bias areas the current tile uses
    if (!(e.dbg & 2)) first_requests(cur, tile, par);
    for (;;) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[x][mb][tb][r] = 0.f;
        if (!(e.dbg & 2)) { if (bsel) k_loop(std::true_type{}, cur); else k_loop(std::false_type{}, cur); }
        const bool more = next_tile(b, tnext);
        if (more) {     // its first patches and U fragments are requested now and land underneath this tile's epilogue
            setup(tnext, cur);
            if (!(e.dbg & 2)) first_requests(cur, tnext, par ^ 1);
        }
        if (e.dbg & 1) { if (acc[0][0][0][0] == 123.456f) e.out[0] = 1.f; }
        else epilogue(tile, par);
        if (!more) break;
        tile = tnext;
        par ^= 1;
    }
#endif
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------
// The transposed bilinear algorithm:  dg[m][c] = G^T [ sum_t (A dY_t A^T) .* (B^T d_t B) ] G  -- per position xi a GEMM
// dU_xi[m][c] = sum_t Z_xi[m][t] V_xi[c][t] over ALL 2x2 output tiles t of all images (K = pixels / 4), then 16 -> 9 values per
// (m, c).  Same 2.25x fewer MFMA operations as the forward.  Workgroup = 64 output channels x 64 input channels, 8 waves, wave w owns
// the positions (a = w >> 1, b in {1, 2} or {0, 3}) as in conv_wino_kernel; a K-slab = 8 tiles of one tile row (2 x 16 output
// pixels): LDS holds the raw 2 x 16 dY patch of the 64 output channels and the raw 4 x 18 X patch of the 64 input channels
// (channel strides 34 / 74 floats: a half-wave's 32 channels read their 8-byte pairs from 64 different banks), ring of 4 stages, LDS-DMA issued by all
// waves (14 dword instructions per wave and slab).  Both MFMA operands are formed from raw values on the fly:
//   Z_ab = sum_pq A[a][p] A[b][q] dY[p][q],  A = [[1,0],[1,1],[1,-1],[0,-1]]  (4 reads, row coefficients are wave constants)
//   V_ab as in the forward (4 or 8 reads).
// The patch moves every slab, so which halo lanes fall off the image is a per-slab scalar (top / bottom / left / right) ANDed with
// per-lane constant bits.  Split-K over the slabs (always: M x C tiles are few), partial dg slabs in [m][c][3][3] order, combined
// by conv_gemm.hip's fixed-order reduce into the gradient bucket.  Bias gradient fused: Z_11 is the sum of a tile's four dY values,
// so the wave that owns position (1, 1) accumulates its A fragments.
constexpr int G_YS = 34, G_XS = 74;                      // channel strides of the dY / X patches (floats): EVEN, = 2 x odd -- the 8-byte
                                                         // reads of a half-wave's 32 channels cover the 64 banks exactly once
constexpr int G_YR = 64 * G_YS / 64, G_XR = 64 * G_XS / 64;   // 64-slot runs of the two regions: 34, 74
constexpr int G_DMA = 14;                                // LDS-DMA instructions per wave and slab (8 x 14 = 112 runs >= 106)
constexpr int G_STAGE = 8 * G_DMA * 64;                  // 7168 floats
constexpr int G_NST = 4;
static_assert(G_NST * G_STAGE >= 16 * 16 * 64, "the exchange buffer lives inside the ring");

struct WinoWgradGeom {
    int batch, C, H, W, M;
    int n_ct, TY, TX;            // input-channel tiles; tile rows per image (H / 2); slabs per tile row (W / 16)
    int n_slab, slabs_per_split; // slabs of the launch (batch * TY * TX)
    int splits, splits_per_xcd;
    int sp_mask, sp_shift;       // fewer than 8 splits (2 or 4): XCD x serves split x & sp_mask and m-tile group x >> sp_shift (-1: off)
    Div dNMT, dNCT, dTX, dTY, dNML;   // dNML: m-tiles per group
    int stack;                   // > 0: dY [1, M, stack * 7, 7] / X [1, C, stack * 7, 7] are stacks of that many 7 x 7 maps (WinoGeom::stack).
                                 // A K-slab = one tile row (of four: rows 2 t, 2 t + 1, row 7 zero) of a PAIR of maps -- 2 x 4 tiles;
                                 // the cursor runs (pair, tile row) with TY = 4, TX = 1; patch columns as in the forward kernel: X
                                 // columns 1 .. 7 and 9 .. 15 are the two maps, 0 / 8 / 16 the zero columns between them, dY column 7 /
                                 // 15 (a map's column 7) zero
};

__global__ __launch_bounds__(512, 2) void conv_wino_wgrad_kernel(const float *__restrict__ dY, const float *__restrict__ X,
                                                                 const WinoWgradGeom g, float *__restrict__ ws, float *__restrict__ db_ws) {
    __shared__ __attribute__((aligned(16))) float lds[G_NST * G_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroup b runs on XCD b % 8: an XCD owns a contiguous run of K-splits and walks ALL (m-tile, c-tile) pairs of a split
    // back to back -- they read the same pixels of dY and X (different channel blocks), so a split's slice of both tensors crosses
    // the fabric once instead of once per tile pair
    int rest, mt, ct, sp;
    if (g.splits_per_xcd > 0) {
        const int x = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
        int sl;
        g.dNMT.divmod(j, rest, mt);
        g.dNCT.divmod(rest, sl, ct);
        sp = x * g.splits_per_xcd + sl;
    } else if (g.sp_shift >= 0) {
        // 2 or 4 splits (512 x 512 channels: 64 tile pairs x 4): an XCD serves ONE split -- a quarter of the pixels -- and one group of
        // the m-tiles with all c-tiles: it reads its pixels of X once and a group's rows of dY (dealt as they come, every XCD read
        // every pixel of X: conv4_2 219 MB for 34 MB of operands)
        const int x = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
        int ml;
        sp = x & g.sp_mask;
        g.dNML.divmod(j, ct, ml);
        mt = ml * (8 >> g.sp_shift) + (x >> g.sp_shift);
    } else {      // tile pairs across the XCDs, as they come
        g.dNMT.divmod((int)blockIdx.x, rest, mt);
        g.dNCT.divmod(rest, sp, ct);
    }
    const int m0 = mt * 64, c0 = ct * 64;
    const int s_begin = sp * g.slabs_per_split, s_end = min(g.n_slab, s_begin + g.slabs_per_split);
    const int plane = g.H * g.W;

    // ---- this wave's LDS-DMA runs: run r = wave * 14 + i covers stage slots [64 r, 64 r + 64) ---------------------------------------
    //   r < 34: dY region, slot = ch * 34 + e, e = p * 16 + col (e >= 32: padding)      34 <= r < 108: X region, slot = ch * 74 + e,
    //   e = row * 18 + col (e >= 72: padding)                                            r >= 108: unused tail of the stage
    unsigned dma_off[G_DMA];
    unsigned long long xbits = 0;     // 4 bits per instruction: the lane's element is in patch row 0 / row 3 / column 0 / column 17
    unsigned pbits = 0;               // 1 bit per instruction: the lane's element lies beyond the image in a row's PARTIAL last slab
    const int rem = g.stack ? 0 : (g.W & 15);         // (W % 16 != 0: that slab holds rem / 2 real tiles; the others see zeros on both operands)
#pragma unroll
    for (int i = 0; i < G_DMA; ++i) {
        const int r = wave * G_DMA + i;
        unsigned off = 0x80000000u;
        if (g.stack) {
            // stacked maps: xbits bit 0 = the element is in a row that does not exist in tile row 0 (X row 0), bit 1 = ... in tile row 3
            // (X rows 2 and 3 = map rows 7 and 8, dY row 1 = map row 7); pbits = the element belongs to the pair's SECOND map
            if (r < G_YR) {
                const int slot = r * 64 + lane, ch = slot / G_YS, e = slot - ch * G_YS;
                const int p = e >> 4, c = e & 15;
                if (e < 32 && m0 + ch < g.M && (c & 7) < 7) {
                    off = (unsigned)((ch * plane + ((c >> 3) * 7 + p) * 7 + (c & 7)) * 4);
                    xbits |= (unsigned long long)((p == 1) << 1) << (4 * i);
                    pbits |= (unsigned)(c >> 3) << i;
                }
            } else if (r < G_YR + G_XR) {
                const int slot = (r - G_YR) * 64 + lane, ch = slot / G_XS, e = slot - ch * G_XS;
                const int row = e / 18, col = e - row * 18;
                if (e < 72 && c0 + ch < g.C && col >= 1 && col <= 16 && ((col - 1) & 7) < 7) {
                    off = (unsigned)((ch * plane + (((col - 1) >> 3) * 7 + row) * 7 + ((col - 1) & 7)) * 4);   // relative to row 2 t - 1: the base is moved back
                    xbits |= (unsigned long long)((row == 0) | ((row >= 2) << 1)) << (4 * i);
                    pbits |= (unsigned)((col - 1) >> 3) << i;
                }
            }
            dma_off[i] = off;
            continue;
        }
        if (r < G_YR) {
            const int slot = r * 64 + lane, ch = slot / G_YS, e = slot - ch * G_YS;
            if (e < 32 && m0 + ch < g.M) {
                off = (unsigned)((ch * plane + (e >> 4) * g.W + (e & 15)) * 4);
                pbits |= (unsigned)((e & 15) >= rem) << i;
            }
        } else if (r < G_YR + G_XR) {
            const int slot = (r - G_YR) * 64 + lane, ch = slot / G_XS, e = slot - ch * G_XS;
            const int row = e / 18, col = e - row * 18;
            if (e < 72 && c0 + ch < g.C) {
                off = (unsigned)((ch * plane + row * g.W + col) * 4);     // relative to (y0 - 1, x0 - 1): the base is moved back
                xbits |= (unsigned long long)((row == 0) | ((row == 3) << 1) | ((col == 0) << 2) | ((col == 17) << 3)) << (4 * i);
                pbits |= (unsigned)(col - 1 >= rem) << i;
            }
        }
        dma_off[i] = off;
    }
    // slab cursor of the issue side: (image, tile row, slab in the row), advanced by one slab per issue; frozen at the last slab
    int q_img, q_ty, q_tx;
    {
        int t;
        g.dTX.divmod(s_begin, t, q_tx);
        g.dTY.divmod(t, q_img, q_ty);
    }
    int q_s = s_begin;
    // one slab's issue, in pieces the K loop spreads over its MFMA slots: the scalars of the slab under the cursor, one instruction
    // at a time (the halo's validity: per-lane constant bits ANDed with the slab's edge scalar -- zero for interior slabs), the advance
    const char *d_yb = nullptr, *d_xb = nullptr;
    int d_soff = 0;
    unsigned d_edge = 0, d_pm = 0;
    auto dma_prepare = [&]() {
        if (g.stack) {      // cursor = (pair q_img, tile row q_ty)
            d_yb = reinterpret_cast<const char *>(dY + (size_t)m0 * plane);
            d_xb = reinterpret_cast<const char *>(X + (size_t)c0 * plane) - 7 * 4;
            d_soff = ((2 * q_img * 7 + 2 * q_ty) * 7) * 4;
            d_edge = (unsigned)(q_ty == 0) | ((unsigned)(q_ty == 3) << 1);
            d_pm = (2 * q_img + 1 >= g.stack) ? pbits : 0u;
            if (q_s + 1 < s_end) {
                ++q_s;
                if (++q_ty == 4) { q_ty = 0; ++q_img; }
            }
            return;
        }
        d_yb = reinterpret_cast<const char *>(dY + ((size_t)q_img * g.M + m0) * plane);
        d_xb = reinterpret_cast<const char *>(X + ((size_t)q_img * g.C + c0) * plane) - (g.W + 1) * 4;
        d_soff = (2 * q_ty * g.W + 16 * q_tx) * 4;
        d_edge = (unsigned)(q_ty == 0) | ((unsigned)(q_ty == g.TY - 1) << 1) | ((unsigned)(q_tx == 0) << 2) | ((unsigned)(q_tx == g.TX - 1) << 3);
        d_pm = (rem != 0 && q_tx == g.TX - 1) ? pbits : 0u;
        if (q_s + 1 < s_end) {
            ++q_s;
            if (++q_tx == g.TX) { q_tx = 0; if (++q_ty == g.TY) { q_ty = 0; ++q_img; } }
        }
    };
    auto dma_one = [&](const int buf, const int i) {
        const unsigned off = (((unsigned)(xbits >> (4 * i)) & d_edge) | ((d_pm >> i) & 1u)) ? 0x80000000u : dma_off[i];
        wino_dma_b32(wave * G_DMA + i < G_YR ? d_yb : d_xb, off, lds + buf * G_STAGE + wave * (G_DMA * 64) + i * 64, d_soff);
    };
    auto issue_dma = [&](const int buf) {
        dma_prepare();
#pragma unroll
        for (int i = 0; i < G_DMA; ++i) dma_one(buf, i);
    };

    // ---- this wave's two positions ------------------------------------------------------------------------------------------------
    // waves w and w + 4 share a SIMD (a workgroup's waves go to the SIMDs cyclically): one of each column set per SIMD -- the {0, 3} waves
    // read and add twice as much per fragment as the {1, 2} waves, and every slab ends in a barrier
    const int a = wave & 3, bsel = wave >> 2;
    const int xi0 = a * 4 + (bsel ? 1 : 0), xi1 = a * 4 + (bsel ? 2 : 3);
    const int i1 = a == 0 ? 0 : a == 2 ? 2 : 1, i2 = a == 0 ? 2 : a == 1 ? 2 : a == 2 ? 1 : 3;     // BT row a (as in the forward)
    const float sgn = a == 1 ? 1.f : -1.f;
    const float ya = a == 3 ? 0.f : 1.f, yb2 = a == 0 ? 0.f : a == 1 ? 1.f : -1.f;                 // A row a = (ya, yb2)
    const int j = lane & 31, h = lane >> 5;
    const int yo = j * G_YS + 2 * h;                          // + mb * 32 * 33 + 4 kp (+ p * 16 + q)
    const int xo = G_YR * 64 + j * G_XS + 2 * h;              // + cb * 32 * 73 + 4 kp + row * 18 (+ column)
    const int xo1 = xo + i1 * 18, xo2 = xo + i2 * 18;
    const bool bias_wave = db_ws != nullptr && ct == 0 && a == 1 && bsel == 1;

    f32x16 acc[2][2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[x][mb][cb][r] = 0.f;
    float rs[2] = {0.f, 0.f};

    // The K loop: the forward kernel's slot pipeline (see there).  Step i = K-pair i (2 tiles): slot m = [MFMA m][a share of: VALU of
    // K-pair i + 1 -- Z = A dY A^T and V = B^T d B on 8-byte register pairs --, the 8-byte ds_reads of K-pair i + 2 into the registers
    // just consumed, one LDS-DMA of slab s + 3]; the hand-over for slab s + 1 behind the first MFMA of step 2.
    auto k_loop = [&](auto bsel_tag) {
        constexpr bool BSEL = decltype(bsel_tag)::value;
        // raw values stay in the 8-byte pairs they are read as; the transforms are written on the pairs (packed fp32 math on
        // natural register pairs -- element-wise code made the compiler assemble pairs with ~50 v_mov per slab)
        wino_f2 ry[2][2], rx[2][4];          // [block][pair]: K-pair i + 1 until consumed, then K-pair i + 2
        float z[2][2][2], v[2][2][2];        // [ring of 2 K-pairs][position][block]
        auto read_y = [&](const float *st, const int kp, const int mb) {
            // 8-byte reads at immediate offsets from three lane addresses (every offset below is a multiple of 2 floats)
#if (SCDA_WINO_ABLATE & 32)
            ry[mb][0] = wino_f2{sgn, ya}; ry[mb][1] = wino_f2{ya, sgn};
            return;
#endif
            const float *p = st + yo + mb * (32 * G_YS) + 4 * kp;
            ry[mb][0] = *reinterpret_cast<const wino_f2 *>(p);          // tile row 0: (q = 0, q = 1)
            ry[mb][1] = *reinterpret_cast<const wino_f2 *>(p + 16);     // tile row 1
        };
        auto read_x = [&](const float *st, const int kp, const int cb) {
#if (SCDA_WINO_ABLATE & 32)
            for (int q = 0; q < 4; ++q) rx[cb][q] = wino_f2{sgn, yb2};
            return;
#endif
            const float *p1 = st + xo1 + cb * (32 * G_XS) + 4 * kp, *p2 = st + xo2 + cb * (32 * G_XS) + 4 * kp;
            rx[cb][0] = *reinterpret_cast<const wino_f2 *>(p1);         // patch row i1: columns (0, 1)
            rx[cb][1] = *reinterpret_cast<const wino_f2 *>(p1 + 2);     //               columns (2, 3)
            rx[cb][2] = *reinterpret_cast<const wino_f2 *>(p2);         // patch row i2
            rx[cb][3] = *reinterpret_cast<const wino_f2 *>(p2 + 2);
        };
        auto valu_z = [&](const int mb, float (&Z)[2][2]) {
            WINO_PIN(ry[mb][0]);
#if (SCDA_WINO_ABLATE & 512)
            Z[0][mb] = ry[mb][0][0]; Z[1][mb] = ry[mb][1][1]; WINO_PIN(Z[0][mb]); WINO_PIN(Z[1][mb]);
            return;
#endif
            const wino_f2 sq = ya * ry[mb][0] + yb2 * ry[mb][1];                      // A row a over the tile's two rows: (s0, s1)
            if (BSEL) { Z[0][mb] = sq[0] + sq[1]; Z[1][mb] = sq[0] - sq[1]; }         // b = 1, 2
            else { Z[0][mb] = sq[0]; Z[1][mb] = -sq[1]; }                             // b = 0, 3
            WINO_PIN(Z[0][mb]);
            WINO_PIN(Z[1][mb]);
        };
        auto valu_v = [&](const int cb, float (&V)[2][2]) {
            WINO_PIN(rx[cb][0]);
#if (SCDA_WINO_ABLATE & 512)
            V[0][cb] = rx[cb][0][0] + rx[cb][2][1]; V[1][cb] = rx[cb][1][0] + rx[cb][3][1]; WINO_PIN(V[0][cb]); WINO_PIN(V[1][cb]);
            return;
#endif
            const wino_f2 p01 = rx[cb][0] + sgn * rx[cb][2], p23 = rx[cb][1] + sgn * rx[cb][3];   // BT row a: (p0, p1), (p2, p3)
            if (BSEL) {
                V[0][cb] = p01[1] + p23[0];       // b = 1: d1 + d2
                V[1][cb] = p23[0] - p01[1];       // b = 2: d2 - d1
            } else {
                const wino_f2 d = p01 - p23;      // b = 0: d0 - d2;  b = 3: d1 - d3
                V[0][cb] = d[0];
                V[1][cb] = d[1];
            }
            WINO_PIN(V[0][cb]);
            WINO_PIN(V[1][cb]);
        };
        auto step = [&](const int kp, const int buf) {
            const float *rst = lds + ((buf + (kp >= 2 ? 1 : 0)) & (G_NST - 1)) * G_STAGE;
            const int rkp = (kp + 2) & 3, rb = kp & 1;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int x = m >> 2, mb = (m >> 1) & 1, cb = m & 1;
                WINO_PIN(v[rb][x][cb]);
                acc[x][mb][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(z[rb][x][mb], v[rb][x][cb], acc[x][mb][cb], 0, 0, 0);
                WINO_PIN(acc[x][mb][cb]);
                if (kp == 2 && m == 0) {
                    // hand-over for the NEXT slab behind an MFMA: this wave's share of its patches has landed (only one slab's issue is younger)
                    __builtin_amdgcn_sched_barrier(0);
                    WINO_WAIT_VMCNT(G_DMA);
#if !(SCDA_WINO_ABLATE & 128)
                    __builtin_amdgcn_s_barrier();
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (kp == 1 && m == 4) dma_prepare();       // (scalar work only: the slab the issue-side cursor is on, ahead of the hand-over)
                if (m == 0 && BSEL && bias_wave) { rs[0] += z[rb][0][0]; rs[1] += z[rb][0][1]; }     // position (1, 1): the tile's four dY values summed
                if (m == 1) { valu_z(0, z[rb ^ 1]); valu_z(1, z[rb ^ 1]); }
                if (m == 2) { read_y(rst, rkp, 0); read_y(rst, rkp, 1); }
                if (m == 3) valu_v(0, v[rb ^ 1]);
                if (m == 4) read_x(rst, rkp, 0);
                if (m == 5) valu_v(1, v[rb ^ 1]);
                if (m == 6) read_x(rst, rkp, 1);
#if !(SCDA_WINO_ABLATE & 64)
                if (kp >= 2) {
                    const int di = (kp - 2) * 8 + m - (kp == 3 ? 1 : 0);      // 14 instructions over the 16 slots of steps 2 and 3
                    if (di >= 0 && di < G_DMA && !(kp == 2 && m == 7)) dma_one((buf + 3) & (G_NST - 1), di);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        issue_dma(0);
        __builtin_amdgcn_sched_barrier(0);
        issue_dma(1);
        __builtin_amdgcn_sched_barrier(0);
        issue_dma(2);
        __builtin_amdgcn_sched_barrier(0);
        WINO_WAIT_VMCNT(2 * G_DMA);
        __builtin_amdgcn_s_barrier();
        {   // fill the pipeline: fragments of K-pair 0, raw values of K-pair 1
#pragma unroll
            for (int b = 0; b < 2; ++b) { read_y(lds, 0, b); read_x(lds, 0, b); }
#pragma unroll
            for (int b = 0; b < 2; ++b) { valu_z(b, z[0]); valu_v(b, v[0]); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < 2; ++b) { read_y(lds, 1, b); read_x(lds, 1, b); }
            __builtin_amdgcn_sched_barrier(0);
        }
        int buf = 0;
        for (int s = s_begin; s < s_end; ++s) {
#pragma unroll
            for (int kp = 0; kp < 4; ++kp) step(kp, buf);
            buf = (buf + 1) & (G_NST - 1);
        }
        WINO_WAIT_VMCNT(0);
    };
    if (bsel) k_loop(std::true_type{}); else k_loop(std::false_type{});

    // ---- epilogue: 4 passes of 16 output-channel rows through LDS, G^T . G, partial dg slab ---------------------------------------------
    const size_t wrow = (size_t)g.C * 9;
#if (SCDA_WINO_ABLATE & 256)
    {
        float tot = 0.f;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot += acc[x][mb][cb][r];
        if (tot == 123.456f) ws[0] = 1.f;
        return;
    }
#endif
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int mb = pass >> 1, half = pass & 1;
        __syncthreads();
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            float *mx = lds + (x ? xi1 : xi0) * (16 * 64) + j;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) {
                    const int r = 8 * half + rr;
                    mx[((r & 3) + 8 * ((r >> 2) & 1) + 4 * h) * 64 + cb * 32] = acc[x][mb][cb][r];
                }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ml = q * 8 + wave, cl = lane;
            const int m = m0 + mb * 32 + half * 16 + ml, c = c0 + cl;
            const float *mp = lds + ml * 64 + cl;
            float t[3][4];     // G^T dU: rows u, columns b
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float d0 = mp[(0 * 4 + b) * 1024], d1 = mp[(1 * 4 + b) * 1024], d2 = mp[(2 * 4 + b) * 1024], d3 = mp[(3 * 4 + b) * 1024];
                t[0][b] = d0 + 0.5f * (d1 + d2);
                t[1][b] = 0.5f * (d1 - d2);
                t[2][b] = 0.5f * (d1 + d2) + d3;
            }
            if (m >= g.M || c >= g.C) continue;
            float *o = ws + ((size_t)sp * g.M + m) * wrow + (size_t)c * 9;
#if (SCDA_WINO_ABLATE & 1024)
            {
                float tot = 0.f;
#pragma unroll
                for (int u = 0; u < 3; ++u) tot += (t[u][0] + 0.5f * (t[u][1] + t[u][2])) + 0.5f * (t[u][1] - t[u][2]) + (0.5f * (t[u][1] + t[u][2]) + t[u][3]);
                if (tot == 123.456f) o[0] = tot;
                continue;
            }
#endif
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                o[u * 3 + 0] = t[u][0] + 0.5f * (t[u][1] + t[u][2]);
                o[u * 3 + 1] = 0.5f * (t[u][1] - t[u][2]);
                o[u * 3 + 2] = 0.5f * (t[u][1] + t[u][2]) + t[u][3];
            }
        }
    }
    if (bias_wave) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const float tsum = rs[mb] + __shfl_xor(rs[mb], 32);
            const int m = m0 + mb * 32 + j;
            if (h == 0 && m < g.M) db_ws[(size_t)sp * g.M + m] = tsum;
        }
    }
}

// ---- transformed weights: wino_pack.h (layout, one tile per workgroup) --------------------------------------------------------------
__global__ __launch_bounds__(256) void wino_pack_kernel(const float *__restrict__ w, float *__restrict__ out, const int Cout, const int Cin,
                                                        const int for_dgrad) {
    __shared__ float tile[16 * 256];
    pack_tile_wino(w, out, Cout, Cin, for_dgrad, (int)blockIdx.x, tile);
}

}  // namespace scda

using namespace scda;

// launch_plan.h DECIDES (route_conv: which convolutions come here; decide_wino / decide_wino_wgrad: tile rows, XCD order, split-K, the
// persistent form); the launchers below check their arguments, build the kernels' geometry from the decision, launch and reduce.
static_assert(lp::WINO_SLAB == WBK && lp::WINO_EPI_PLAIN == WEPI_PLAIN && lp::WINO_EPI_MASK == WEPI_MASK && lp::WINO_EPI_POOL == WEPI_POOL &&
              lp::WINO_EPI_SPLIT == WEPI_SPLIT, "launch_plan.h restates the kernels' constants");

SCDA_API int scda_conv2d_wino_supported(int batch, int C, int H, int W, int M) { return lp::wino_kernel_ok(batch, C, H, W, M, 0); }

SCDA_API int scda_conv2d_wino_wgrad_supported(int batch, int Cin, int H, int W, int Cout) {
    return lp::wino_wgrad_kernel_ok(batch, Cin, H, W, Cout, 0);
}

SCDA_API int scda_conv2d_wino_enabled(void) { return lp::read_wino_env().enabled; }

SCDA_API int scda_conv2d_route(int dir, int batch, int Cin, int IH, int IW, int Cout, int KH, int KW, int S, int P, int row_period,
                               int *pool, int *maps) {
    const lp::ConvRoute r = lp::route_conv(dir, lp::ConvShape{batch, Cin, IH, IW, Cout, KH, KW, S, P, row_period}, lp::read_wino_env());
    if (pool) *pool = r.pool;
    if (maps) *maps = r.maps;
    return r.family;
}

SCDA_API size_t scda_conv2d_wino_packed_elems(int Cout, int Cin, int for_dgrad) {
    return (size_t)wino_packed_elems(for_dgrad ? Cin : Cout, for_dgrad ? Cout : Cin);
}

SCDA_API int scda_conv2d_wino_pack_hip(const float *w, float *out, int Cout, int Cin, int for_dgrad, void *stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || ((for_dgrad ? Cout : Cin) % WBK) != 0) { set_error("scda_conv2d_wino_pack_hip: bad arguments"); return SCDA_EINVAL; }
    const long long tiles = wino_pack_tiles(for_dgrad ? Cin : Cout, for_dgrad ? Cout : Cin);
    hipLaunchKernelGGL(wino_pack_kernel, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), w, out, Cout, Cin, for_dgrad ? 1 : 0);
    return launch_status("wino_pack_kernel");
}

// test aid (scda_debug_wino_last_order / _last_persistent): what the calling thread's most recent launches were decided to be
static thread_local struct { lp::WinoDecision fwd; lp::WinoWgradDecision wgrad; } g_wino_last;

SCDA_API int scda_debug_wino_last_persistent(void) { return g_wino_last.fwd.persist; }

SCDA_API void scda_debug_wino_last_order(int *out6) {
    const lp::WinoDecision &d = g_wino_last.fwd;
    out6[0] = d.mb; out6[1] = d.pixel_major; out6[2] = d.gm; out6[3] = d.splits;
    out6[4] = g_wino_last.wgrad.splits; out6[5] = g_wino_last.wgrad.order;
}

// both decisions of one layer for a 256-CU device, their ints in declaration order; nothing is launched or allocated
SCDA_API void scda_debug_plan_wino(int batch, int C, int H, int W, int M, int stack, int pool, int masked, int with_db, size_t ws_bytes,
                                   int *fwd9, int *wgrad6) {
    static_assert(sizeof(lp::WinoDecision) == 9 * sizeof(int) && sizeof(lp::WinoWgradDecision) == 6 * sizeof(int), "scda_ops.h documents 9 + 6 ints");
    const lp::WinoEnv env = lp::read_wino_env();
    const lp::WinoDecision f = lp::decide_wino(batch, C, H, W, M, stack, pool != 0, masked != 0, ws_bytes, 256, env);
    const lp::WinoWgradDecision w = lp::decide_wino_wgrad(batch, C, H, W, M, stack, with_db != 0, ws_bytes, env);
    memcpy(fwd9, &f, sizeof f);
    memcpy(wgrad6, &w, sizeof w);
}

// evidence aid (scripts/pmc_summary.py): SCDA_WINO_LOG=<file> appends one line per launch of the three kernels, in launch order --
// kind, tile rows / 32, workgroups, shape, split count and the launch's ALGORITHMIC bytes (operands once + result once) -- so that
// a counter pass's dispatches can be joined with the layers they ran.  The file named at the first launch is the one kept.
static void wino_log(const char *path, const char *kind, int mb, long long wgs, int batch, int C, int H, int W, int M, int splits, double bytes,
                     double flops) {
    static FILE *f = path && *path ? fopen(path, "a") : nullptr;
    if (!f) return;
    fprintf(f, "%s %d %lld %d %d %d %d %d %d %.0f %.0f\n", kind, mb, wgs, batch, C, H, W, M, splits, bytes, flops);
    fflush(f);
}

// y [batch, M, H, W] = act(conv3x3(x [batch, C, H, W], stride 1, pad 1) + bias) (* act'(mask_src)); u = scda_conv2d_wino_pack_hip
static int wino_launch(const float *x, const float *u, const float *bias, float *y, int batch, int C, int H, int W, int M, int act,
                       float slope, const float *mask_src, float mask_slope, int for_dgrad, void *ws, size_t ws_bytes, void *stream,
                       float *pool_y, unsigned char *pool_idx, int stack = 0) {
    if (!x || !u || (!y && !pool_y)) { set_error("scda_conv2d_wino_hip: bad arguments"); return SCDA_EINVAL; }
    if (!lp::wino_kernel_ok(batch, C, H, W, M, stack) || (stack && pool_y)) {
        set_error("scda_conv2d_wino_hip: needs C %% 8 == 0, even H and W (or a stack of 7 x 7 maps) and tensors below 2 GB per image (C=%d H=%d W=%d)", C, H, W);
        return SCDA_EINVAL;
    }
    hipStream_t st = as_stream(stream);
    static const int n_cu = [] { int d = 0, n = 0; if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n < 8) n = 256; return n / 8 * 8; }();
    const lp::WinoEnv env = lp::read_wino_env();
    const lp::WinoDecision d = lp::decide_wino(batch, C, H, W, M, stack, pool_y != nullptr, mask_src != nullptr, ws_bytes, n_cu, env);
    g_wino_last.fwd = d;
    const lp::WinoBlocks b = lp::wino_blocks(batch, H, W, stack);      // blocks on the right / bottom edge may be partial
    WinoGeom g;
    g.batch = batch; g.C = C; g.H = H; g.W = W; g.M = M; g.stack = stack;
    g.n_mbg = (M + 63) / 64 * 2;
    g.n_mt = (M + 32 * d.mb - 1) / (32 * d.mb); g.n_slab = C / WBK; g.slabs_per_split = d.slabs_per_split;
    g.dNMT = Div(g.n_mt); g.dNPB = Div(b.npb); g.dNB = Div(b.nby * b.nbx); g.dNBX = Div(b.nbx);
    g.pixel_major = d.pixel_major; g.npb = b.npb; g.per_xcd = d.per_xcd; g.n_wg = d.n_wg;
    g.gm_mask = d.gm - 1; g.gm_shift = d.gm == 4 ? 2 : d.gm == 2 ? 1 : 0;
    g.dNML = Div(g.n_mt / d.gm);
    WinoEpi e{y, (float *)ws, bias, act, slope, d.splits, mask_src, mask_slope, env.dbg, pool_y, pool_idx};
    // flops = the MFMA work the kernel EXECUTES (16 products per 2x2 tile and channel pair: the direct form's 36 / 2.25)
    // algorithmic bytes: input once, filters once, result once (fused pool: the pooled map and its winners instead of the full map)
    const double out_bytes = pool_y ? 1.25 * batch * M * H * W : 4.0 * batch * M * H * W, flops = 2.0 * M * (double)batch * H * W * C * 4;
    const double alg_bytes = 4.0 * ((double)batch * C * H * W + 9.0 * M * C) + out_bytes + (mask_src ? 4.0 * batch * M * H * W : 0.0);   // (+ the activation mask)
    prof_begin(for_dgrad ? PK_WINO_DGRAD : PK_WINO_FWD, flops, st, alg_bytes);
    wino_log(env.log, pool_y ? "fwd_pool" : for_dgrad ? (mask_src ? "dgrad_mask" : "dgrad") : "fwd", d.mb, d.n_wg, batch, C, H, W, M, d.splits, alg_bytes, flops);
#define WINO_LAUNCH(MB_, P_, E_) hipLaunchKernelGGL((conv_wino_kernel<MB_, P_, E_>), dim3((unsigned)((P_) ? n_cu : d.n_wg)), dim3(512), 0, st, u, x, g, e)
#define WINO_LAUNCH_EPI(MB_, P_)                                                      \
    do {                                                                              \
        if (d.epi == WEPI_SPLIT) {                                                    \
            if (P_) { prof_end(st); set_error("conv_wino_kernel: a split launch cannot be persistent"); return SCDA_EINVAL; } \
            WINO_LAUNCH(MB_, false, WEPI_SPLIT);                                      \
        }                                                                             \
        else if (d.epi == WEPI_POOL) WINO_LAUNCH(MB_, P_, WEPI_POOL);                 \
        else if (d.epi == WEPI_MASK) WINO_LAUNCH(MB_, P_, WEPI_MASK);                 \
        else WINO_LAUNCH(MB_, P_, WEPI_PLAIN);                                        \
    } while (0)
    if (d.persist) WINO_LAUNCH_EPI(2, true);       // (a persistent launch never splits: it has more tiles than CUs)
    else if (d.mb == 2) WINO_LAUNCH_EPI(2, false);
    else WINO_LAUNCH_EPI(1, false);
#undef WINO_LAUNCH_EPI
#undef WINO_LAUNCH
    prof_end(st);
    int rc = launch_status("conv_wino_kernel");
    if (rc || d.splits == 1) return rc;
    return launch_conv_reduce((const float *)ws, d.splits, M, batch * H * W, H * W, bias, act, slope, y, mask_src, mask_slope, st);
}

SCDA_API int scda_conv2d_wino_hip(const float *x, const float *u, const float *bias, float *y, int batch, int C, int H, int W, int M,
                                  int act, float slope, const float *mask_src, float mask_slope, int for_dgrad, void *ws, size_t ws_bytes,
                                  void *stream) {
    return wino_launch(x, u, bias, y, batch, C, H, W, M, act, slope, mask_src, mask_slope, for_dgrad, ws, ws_bytes, stream, nullptr, nullptr);
}

// the same on x [1, C, maps * 7, 7] read as a vertical stack of `maps` independent 7 x 7 maps (row period 7: no tap reaches from one
// map into the next) -- the 3x3 convolutions of the ResNet-50 C4 detector's channel-major RoI head (models/mask_rcnn/resnet.py:131-148)
SCDA_API int scda_conv2d_wino_stacked_hip(const float *x, const float *u, const float *bias, float *y, int maps, int C, int M, int act,
                                          float slope, const float *mask_src, float mask_slope, int for_dgrad, void *ws, size_t ws_bytes,
                                          void *stream) {
    return wino_launch(x, u, bias, y, 1, C, maps * 7, 7, M, act, slope, mask_src, mask_slope, for_dgrad, ws, ws_bytes, stream, nullptr, nullptr, maps);
}

// conv3x3 + bias + activation + 2x2/2 max-pool in one launch: pool_y [batch, M, H/2, W/2] and pool_idx (uint8, winner 0..3 as
// scda_maxpool2x2_fwd_hip writes it) -- the full-resolution map is never written (vgg_adver_expansion_cluster.py:101-114: the pools
// behind conv1_2 / conv2_2 / conv3_3 / conv4_3).  A Winograd tile IS a pooling window.
SCDA_API int scda_conv2d_wino_pool_hip(const float *x, const float *u, const float *bias, float *pool_y, unsigned char *pool_idx, int batch,
                                       int C, int H, int W, int M, int act, float slope, void *stream) {
    if (!pool_y || !pool_idx) { set_error("scda_conv2d_wino_pool_hip: bad arguments"); return SCDA_EINVAL; }
    return wino_launch(x, u, bias, nullptr, batch, C, H, W, M, act, slope, nullptr, 0.f, 0, nullptr, 0, stream, pool_y, pool_idx);
}

static int wino_wgrad_launch(const float *dy, const float *x, float *dw, float *db, int batch, int Cin, int H, int W, int Cout,
                             int accumulate, int db_accumulate, void *ws, size_t ws_bytes, void *stream, int stack) {
    if (!dy || !x || !dw || !ws) { set_error("scda_conv2d_wino_wgrad_hip: bad arguments"); return SCDA_EINVAL; }
    if (!lp::wino_wgrad_kernel_ok(batch, Cin, H, W, Cout, stack)) {
        set_error("scda_conv2d_wino_wgrad_hip: needs >= 32 channels on both sides (>= 64 on stacked maps) and even H, W or a stack of 7 x 7 maps (Cin=%d Cout=%d H=%d W=%d)", Cin, Cout, H, W);
        return SCDA_EINVAL;
    }
    if (ws_bytes < ((size_t)Cin * 9 + (db ? 1024 : 0)) * Cout * sizeof(float)) { set_error("scda_conv2d_wino_wgrad_hip: workspace too small"); return SCDA_EINVAL; }
    hipStream_t st = as_stream(stream);
    const lp::WinoEnv env = lp::read_wino_env();
    const lp::WinoWgradDecision d = lp::decide_wino_wgrad(batch, Cin, H, W, Cout, stack, db != nullptr, ws_bytes, env);
    g_wino_last.wgrad = d;
    const int n_mt = (Cout + 63) / 64;
    WinoWgradGeom g;
    g.batch = batch; g.C = Cin; g.H = H; g.W = W; g.M = Cout; g.stack = stack;
    g.n_ct = (Cin + 63) / 64; g.TY = stack ? 4 : H / 2; g.TX = stack ? 1 : (W + 15) / 16;
    g.n_slab = d.n_slab; g.slabs_per_split = d.slabs_per_split;
    g.dNMT = Div(n_mt); g.dNCT = Div(g.n_ct); g.dTX = Div(g.TX); g.dTY = Div(g.TY);
    g.splits = d.splits; g.splits_per_xcd = d.splits_per_xcd;
    g.sp_mask = 0; g.sp_shift = -1; g.dNML = Div(1);
    if (d.order == 2) {
        g.sp_mask = d.splits - 1; g.sp_shift = d.splits == 4 ? 2 : 1;
        g.dNML = Div(n_mt / (8 / d.splits));
    }
    float *wsf = (float *)ws;
    float *db_ws = db ? wsf + (size_t)d.splits * Cout * Cin * 9 : nullptr;
    const double flops = 2.0 * Cout * (double)batch * H * W * Cin * 4;
    prof_begin(PK_WINO_WGRAD, flops, st);
    wino_log(env.log, "wgrad", 2, d.grid, batch, Cin, H, W, Cout, d.splits, 4.0 * ((double)batch * (Cin + Cout) * H * W + 9.0 * Cout * Cin), flops);
    hipLaunchKernelGGL(conv_wino_wgrad_kernel, dim3((unsigned)d.grid), dim3(512), 0, st, dy, x, g, wsf, db_ws);
    prof_end(st);
    int rc = launch_status("conv_wino_wgrad_kernel");
    if (rc) return rc;
    return launch_wgrad_reduce(wsf, d.splits, (long long)Cout * Cin * 9, Cin * 9, accumulate, dw, db_ws, db, Cout, db_accumulate, st);
}

// dw [Cout,Cin,3,3] (+)= weight gradient of the stride-1, pad-1 3x3 convolution; db [Cout] (+)= bias gradient (may be NULL)
SCDA_API int scda_conv2d_wino_wgrad_hip(const float *dy, const float *x, float *dw, float *db, int batch, int Cin, int H, int W, int Cout,
                                        int accumulate, int db_accumulate, void *ws, size_t ws_bytes, void *stream) {
    return wino_wgrad_launch(dy, x, dw, db, batch, Cin, H, W, Cout, accumulate, db_accumulate, ws, ws_bytes, stream, 0);
}

// ... on dy [1, Cout, maps * 7, 7] / x [1, Cin, maps * 7, 7] read as stacks of `maps` independent 7 x 7 maps (scda_conv2d_wino_stacked_hip)
SCDA_API int scda_conv2d_wino_wgrad_stacked_hip(const float *dy, const float *x, float *dw, float *db, int maps, int Cin, int Cout,
                                                int accumulate, int db_accumulate, void *ws, size_t ws_bytes, void *stream) {
    return wino_wgrad_launch(dy, x, dw, db, 1, Cin, maps * 7, 7, Cout, accumulate, db_accumulate, ws, ws_bytes, stream, maps);
}
