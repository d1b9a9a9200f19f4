// launch_plan.h -- which kernel family, tile, split-K count, tile order and grid every convolution, weight gradient and dense
// GEMM runs with; which convolutions take the Winograd kernels instead (route_conv) and how those launch (decide_wino,
// decide_wino_wgrad).  Host arithmetic only (plain C++17, no HIP): conv_gemm.hip and conv_wino.hip ask one decide_* function per
// launch and launch what the decision names; scda_debug_plan_conv / scda_debug_plan_gemm / scda_debug_plan_wino return the same
// structs and scda_conv2d_route the route without a GPU (tests/test_launch_plans.py pins them against tests/golden/launch_plans.json
// and wino_plans.json).  Every environment variable of these paths is read here, in read_plan_env / read_wino_env.
#ifndef SCDA_LAUNCH_PLAN_H
#define SCDA_LAUNCH_PLAN_H

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace scda {
namespace lp {

constexpr int BK = 16;                       // K-slab depth of every MFMA kernel (mfma_tile.h)
constexpr int X9_BM = 256, X9_BN = 128;      // the bf16 x 9 kernel's one tile (GemmX9Cfg)

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int conv_out_dim(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }
static inline int conv_packed_mpad(int M) { return M <= 64 ? 64 : (M + 127) / 128 * 128; }   // as conv_gemm.hip packs the weights

// ----------------------------- environment: the launch-plan tools, each read in ONE place --------------------------
struct ForcedPlan { bool set; int bm, bn, splits; };
struct PlanEnv {
    ForcedPlan force;        // SCDA_PLAN_FORCE="bm,bn,splits": tuning / test aid for every launch (scripts/tune_plans.py)
    bool allow_bm64;         // SCDA_PLAN_ALLOW_BM64: a forced 64-row tile is legal on problems of more than 64 rows
    const char *override_;   // SCDA_PLAN_OVERRIDE="M,N,K:bm,bn,splits;...": individual shapes, inside the real iteration
    bool log;                // SCDA_PLAN_LOG: one "[scda plan]" line per newly planned shape
    int x9_mode;             // SCDA_GEMM_X9: 0 never, 2 whatever its size (tests), default 1: the FC-sized products
    int x9_sk;               // SCDA_GEMM_X9_SK: 0 one workgroup per tile, 2 stream-K for any tile count, default 1: more tiles than CUs
    int x9_splits;           // SCDA_GEMM_X9_SPLITS: forced split-K count of the bf16 x 9 kernel (0: not set)
    bool x9_splits_set;
};

// (read per call: the tests switch these between launches)
static PlanEnv read_plan_env() {
    PlanEnv e{};
    if (const char *f = getenv("SCDA_PLAN_FORCE")) e.force.set = sscanf(f, "%d,%d,%d", &e.force.bm, &e.force.bn, &e.force.splits) == 3;
    e.allow_bm64 = getenv("SCDA_PLAN_ALLOW_BM64") != nullptr;
    e.override_ = getenv("SCDA_PLAN_OVERRIDE");
    e.log = getenv("SCDA_PLAN_LOG") != nullptr;
    const char *x9 = getenv("SCDA_GEMM_X9"), *sk = getenv("SCDA_GEMM_X9_SK"), *sp = getenv("SCDA_GEMM_X9_SPLITS");
    e.x9_mode = x9 ? atoi(x9) : 1;
    e.x9_sk = sk ? atoi(sk) : 1;
    e.x9_splits_set = sp != nullptr;
    e.x9_splits = sp ? atoi(sp) : 0;
    return e;
}

// ----------------------------- the occupancy model --------------------------
// Launch plan = (N-tile width, split-K count), chosen with a small occupancy model instead of fixed thresholds.
// At these sizes a launch has only a few workgroups per CU, so WAVE QUANTISATION decides the speed: the direct-to-LDS
// kernels keep 64 KB (128x128), 48 KB (128x64 / 64x128) or 32 KB (64x64) of LDS per workgroup = 2 / 3 / 4 resident per CU, a
// CU needs >= 2 resident workgroups (2 waves per SIMD) to keep its MFMA pipe fed across the per-slab barrier, and a CU
// that is left with ONE workgroup runs it at about half speed.  Measured: the conv3_2 weight gradient at 756 workgroups
// (2.95 per CU -> a round of two, then a round of one) ran at 81 TFLOP/s, at 504 (one round of two) 101 TFLOP/s.
//   time(plan) = flops / (model efficiency x 110 TFLOP/s) + split-K slab traffic (write + read) at 3 TB/s
struct LaunchPlan { int bn, splits, bm; };

// what one caller's kernels can run: the candidate tiles of the search AND the legality of a forced plan
struct TileRules {
    int bm;                  // natural tile rows (64 for problems of <= 64 rows, else 128)
    bool allow64, allow128, allow256;   // N-tile widths
    bool allow_bm256;        // the 8-wave 256 x 128 tile
    int bn32;                // width of the 32-row tile where this problem may run it (0: not legal here).  Never searched: the callers
                             // take it by rule, or when it is forced
    bool one_pass32;         // ... which has no split-K form (forward / data gradient)
    bool must_split;         // the kernel always writes slabs (weight gradient)
    int k_granule;           // K-steps come in multiples of this
    bool one_tap;            // 1x1 convolution on the direct-to-LDS kernel (tile_efficiency_one_tap)
};

static int resident_per_cu(int bm, int bn) { return bm == 256 ? 1 : ((bm == 128 && bn == 128) || bn == 256) ? 2 : (bm == 64 && bn == 64) ? 4 : 3; }
static double tile_efficiency(int bm, int bn) { return bm == 256 ? 1.05 : ((bm == 128 && bn == 128) || bn == 256) ? 1.0 : (bm == 64 && bn == 64) ? 0.85 : 0.90; }
// 1x1 convolutions (one filter tap): a K-slab never re-reads lines the previous slabs brought into L1 / L2 (a 3x3 layer's nine taps
// of a channel group are consecutive slabs over the same input lines), every gather is a fresh L2 / HBM access, and what hides that
// latency is the number of independent workgroups per CU, not the MFMA work per barrier: brute force over the ResNet-50 shapes
// (scripts/tune_plans.py resnet) has the 64x64 tile (4 resident per CU) ahead of the 8-wave 256x128 tile by 7 - 23 % on EVERY 1x1
// forward / data-gradient layer (head 512 -> 2048 on 25088 pixels: 470 vs 561 us), and level with it on every 3x3 layer.
static double tile_efficiency_one_tap(int bm, int bn) { return (bm == 64 && bn == 64) ? 1.0 : (bm == 64 || (bm == 128 && bn == 64)) ? 0.9 : 0.85; }

// time, in units of one workgroup running at full CU speed, for the busiest CU to finish c workgroups with p resident
static double cu_rounds(int c, int p, bool eight_waves = false) {
    if (eight_waves) return (double)c;   // an 8-wave workgroup keeps the CU's MFMA pipes fed on its own
    double t = 0;
    while (c > 0) {
        const int r = c < p ? c : p;
        t += r == 1 ? 2.0 : (double)r;
        c -= r;
    }
    return t;
}

static double plan_cost(long long tiles, int splits, int bm, int bn, double flops, double out_bytes, bool one_tap = false) {
    const long long wgs = tiles * splits;
    const double ideal = (double)wgs / 256.0;
    const double eff = ideal / cu_rounds(cdiv(wgs, 256), resident_per_cu(bm, bn), bm == 256) * (one_tap ? tile_efficiency_one_tap(bm, bn) : tile_efficiency(bm, bn));
    double t = flops / (eff * 110e12);
    if (splits > 1) t += 2.0 * splits * out_bytes / 3e12;
    return t;
}

// ----------------------------- rules every caller shares --------------------------
// the largest split count <= splits whose [splits][M][N] slabs fit the workspace
static int fit_splits(int splits, int M, int N, size_t ws_bytes) {
    while (splits > 1 && (size_t)splits * M * N * sizeof(float) > ws_bytes) --splits;
    return splits;
}

static int round_k_per_split(int K, int splits) {
    int kps = (K + splits - 1) / splits;
    kps = (kps + BK - 1) / BK * BK;
    return kps;
}

// grouped tile order (tile_coords, swz bit 1: 8 M-tiles at a time across all N-tiles): many M-tiles whose A panels together do not
// fit an XCD's L2 but a quarter of them does.  The ResNet RoI head's 512 -> 2048 1x1: 32 weight panels = 4.2 MB, walked M-tile-fastest
// they were re-fetched for every pixel tile (762 MB read for a 51 MB input); FC6's weight gradient: 8 MB of dY re-read per column.
static bool grouped_tile_order(int nx, int ny, int M, int K) {
    return ny >= 16 && (long long)nx * ny >= 1024 && (double)M * K * sizeof(float) > 4e6;
}

// THE legality test of a forced plan (SCDA_PLAN_FORCE and SCDA_PLAN_OVERRIDE): a tile the caller's kernels have, slabs that fit
// the workspace, and (cap_k) at least two K-steps per split
static bool forced_plan_legal(const TileRules &r, const ForcedPlan &f, int M, int N, int K, size_t ws_bytes, bool bm64_ok, bool cap_k) {
    if (f.splits < 1 || (f.splits > 1 && (size_t)f.splits * M * N * sizeof(float) > ws_bytes)) return false;
    if (cap_k && f.splits > std::max(1, K / (r.k_granule * 2))) return false;
    if (f.bm == 32) return r.bn32 != 0 && f.bn == r.bn32 && !(r.one_pass32 && f.splits != 1);
    const bool rows = f.bm == r.bm || (f.bm == 256 && r.allow_bm256) || (f.bm == 64 && bm64_ok && !r.must_split);
    const bool cols = (f.bn == 64 && r.allow64) || (f.bn == 128 && r.allow128) || (f.bn == 256 && r.allow256);
    return rows && cols && !(f.bm == 256 && f.bn != 128);
}

static LaunchPlan plan_search(int M, int N, int K, const TileRules &r, size_t ws_bytes) {
    const double flops = 2.0 * M * (double)N * K, out_bytes = (double)M * N * sizeof(float);
    double best_t = 1e30;
    int max_s = K / (r.k_granule * 4);   // at least 4 K-steps per split
    if (max_s < 1) max_s = 1;
    if (max_s > 256) max_s = 256;
    max_s = fit_splits(max_s, M, N, ws_bytes);
    LaunchPlan best{r.allow128 ? 128 : 64, 1, r.bm};
    // tile-row candidates: the natural one; 256 (8 waves) where legal; 64 for 65..128-row problems (the decoder's 128-channel
    // layers: 512 half-height tiles and no split-K beat 128 full tiles split four ways by ~6 %)
    // ... and for 1x1 convolutions of any height (tile_efficiency_one_tap)
    const bool allow_bm64 = r.bm == 128 && (M <= 128 || r.one_tap) && r.allow64 && !r.must_split && r.k_granule == BK;
    for (int pass = 0; pass < 3; ++pass) {
        if ((pass == 1 && !r.allow_bm256) || (pass == 2 && !allow_bm64)) continue;
        const int tbm = pass == 1 ? 256 : pass == 2 ? 64 : r.bm;
        for (int bn = 64; bn <= 256; bn *= 2) {
            if ((bn == 64 && !r.allow64) || (bn == 128 && !r.allow128) || (bn == 256 && !r.allow256)) continue;
            if (tbm == 256 && bn != 128) continue;
            const long long tiles = (long long)cdiv(M, tbm) * cdiv(N, bn);
            for (int sp = 1; sp <= max_s; ++sp) {
                if (tiles * sp > 4096 && sp > 1) break;   // plenty of workgroups already: splitting only adds traffic
                double t = plan_cost(tiles, sp, tbm, bn, flops, out_bytes, r.one_tap);
                if (r.must_split && sp == 1) t += 2.0 * out_bytes / 3e12;
                if (t < best_t) { best_t = t; best = LaunchPlan{bn, sp, tbm}; }
            }
        }
    }
    return best;
}

// a legal forced plan, else the model's; memoised per thread (the same ~60 shapes recur every iteration; launches come from the
// main and the autograd thread)
static LaunchPlan plan_tiles(int M, int N, int K, const TileRules &r, size_t ws_bytes, const PlanEnv &env) {
    if (env.force.set && forced_plan_legal(r, env.force, M, N, K, ws_bytes, env.allow_bm64, true))
        return LaunchPlan{env.force.bn, env.force.splits, env.force.bm};
    for (const char *q = env.override_; q && *q;) {
        int m = 0, n = 0, k = 0;
        ForcedPlan f{true, 0, 0, 0};
        if (sscanf(q, "%d,%d,%d:%d,%d,%d", &m, &n, &k, &f.bm, &f.bn, &f.splits) == 6 && m == M && n == N && k == K && !r.must_split &&
            forced_plan_legal(r, f, M, N, K, ws_bytes, true, false))
            return LaunchPlan{f.bn, f.splits, f.bm};
        q = strchr(q, ';');
        if (q) ++q;
    }
    struct Key { int M, N, K, flags; size_t ws; };
    struct Entry { Key k; LaunchPlan p; };
    static thread_local std::vector<Entry> cache;
    const Key key{M, N, K, r.bm | (r.allow64 << 8) | (r.allow128 << 9) | (r.must_split << 10) | (r.allow256 << 11) | (r.k_granule << 12) | (r.allow_bm256 << 20) | (r.one_tap << 21), ws_bytes};
    for (const Entry &e : cache)
        if (e.k.M == key.M && e.k.N == key.N && e.k.K == key.K && e.k.flags == key.flags && e.k.ws == key.ws) return e.p;
    const LaunchPlan p = plan_search(M, N, K, r, ws_bytes);
    if (env.log)
        fprintf(stderr, "[scda plan] M=%d N=%d K=%d %s-> tile %dx%d splits %d (%lld workgroups)\n", M, N, K, r.must_split ? "wgrad " : "",
                p.bm, p.bn, p.splits, (long long)cdiv(M, p.bm) * cdiv(N, p.bn) * p.splits);
    if (cache.size() < 512) cache.push_back(Entry{key, p});
    return p;
}

// ----------------------------- the complete decision of one launch --------------------------
enum Family {
    FAM_STAGED = 0,       // register-staged kernels (any shape / alignment)
    FAM_GLDS = 1,         // direct-to-LDS kernels (whole 16-deep slabs, 16-byte addressable rows)
    FAM_X9 = 2,           // exact-product bf16 x 9 GEMM
    FAM_SMALL_CIN = 3,    // image-side 3x3 forward, Cin <= 4: the direct kernel (no tiles)
};

struct LaunchDecision {
    int family;
    int x9_stream;        // FAM_X9: the persistent stream-K launch (grid = one workgroup per CU)
    int bm, bn, splits, k_per_split;
    int nx, ny, grid;     // tile grid and workgroups of the launch
    int swz;              // tile_coords: bit 0 XCD-contiguous ids, bit 1 grouped tile order
    int parity, nc, ncp;  // stride-2 data gradient: parity classes (ConvGeom::parity)
    int wbk;              // register-staged weight gradient: K-slab depth 16 / 32
    int reduce;           // a second launch follows: the split-K reduce, or the stream-K fix-up
    int x9_r;             // stream-K: (tile, slab) units per workgroup
};

// what scda_debug_last_plan reports as the kernel family: 1 direct-to-LDS, 2 bf16 x 9, 0 otherwise
static int reported_family(const LaunchDecision &d) { return d.family == FAM_GLDS ? 1 : d.family == FAM_X9 ? 2 : 0; }

// one convolution as the entry points receive it
struct ConvShape {
    int batch, Cin, IH, IW, Cout, KH, KW, S, P, row_period;
    int OH() const { return conv_out_dim(IH, KH, S, P); }
    int OW() const { return conv_out_dim(IW, KW, S, P); }
    bool gemm_1x1() const { return batch == 1 && KH == 1 && KW == 1 && S == 1 && P == 0; }   // a dense GEMM on the NCHW tensors as they lie
};

// ----------------------------- bf16 x 9 GEMM --------------------------
// n_cu: persistent workgroups of the stream-K form (the device's CU count, a multiple of 8)
static LaunchDecision decide_gemm_x9(int M, int N, int K, int ldc, size_t ws_bytes, int n_cu, const PlanEnv &env) {
    LaunchDecision d{};
    d.family = FAM_X9; d.bm = X9_BM; d.bn = X9_BN;
    d.nx = cdiv(N, X9_BN); d.ny = cdiv(M, X9_BM);
    const long long tiles = (long long)d.nx * d.ny;
    // more tiles than CUs: the persistent stream-K form (SCDA_GEMM_X9_SK=0 keeps one workgroup per tile, =2 forces it for any count)
    const size_t slot_bytes = (size_t)2 * n_cu * X9_BM * X9_BN * sizeof(float);
    d.x9_stream = !env.x9_splits_set && ws_bytes >= slot_bytes && (env.x9_sk == 2 || (env.x9_sk == 1 && tiles > n_cu));
    // split-K (one workgroup per (tile, split)): fill the CUs when there are fewer tiles than CUs (>= 32 slabs per split);
    // SCDA_GEMM_X9_SPLITS forces a count
    int splits = 1;
    if (env.x9_splits_set) splits = env.x9_splits;
    else if (!d.x9_stream && tiles < 200) splits = (int)std::min<long long>((256 + tiles / 2) / tiles, std::max(1, K / BK / 32));
    if (splits < 1) splits = 1;
    if (ldc != N) splits = 1;
    splits = fit_splits(splits, M, N, ws_bytes);
    d.k_per_split = round_k_per_split(K, splits);
    d.splits = cdiv(K, d.k_per_split);
    d.swz = 1 | (grouped_tile_order(d.nx, d.ny, M, K) ? 2 : 0);
    if (d.x9_stream) {
        const long long units = tiles * (K / BK);
        d.x9_r = (int)((units + n_cu - 1) / n_cu);
        d.grid = n_cu;
        d.reduce = !(units % d.x9_r == 0 && d.x9_r % (K / BK) == 0);   // every range is whole tiles: nothing was cut, no fix-up
    } else {
        d.grid = (int)(tiles * d.splits);
        d.reduce = d.splits > 1;
    }
    return d;
}

// may this product run on the direct-to-LDS GEMM kernels (whole 16-deep slabs, 16-byte addressable rows, 32-bit lane offsets:
// 256 rows of either operand stay below 2 GB)?  aligned: both operand pointers are 16-byte aligned
static bool gemm_glds_operands_ok(bool aligned, int M, int N, int K, int lda, int ldb, int trans_a, int trans_b) {
    return (K % BK) == 0 && (lda % 4) == 0 && (ldb % 4) == 0 && aligned &&
           (!trans_a || (M % 4) == 0) && (!trans_b || (N % 4) == 0) && (long long)lda * 1024 + (long long)M * 4 < (1LL << 31) &&
           (long long)ldb * 1024 + (long long)N * 4 < (1LL << 31);
}

// should it take the exact-product bf16 x 9 kernel?  Default: the FC-sized ones
static bool gemm_x9_wanted(int M, int N, int K, const PlanEnv &env) {
    if (env.force.set) return false;      // a forced (tile, split) plan names an fp32-MFMA instantiation: that one runs
    return env.x9_mode == 2 || (env.x9_mode == 1 && M >= 256 && N >= 128 && K >= 256 && (double)M * N * K >= 4e9);
}

// ----------------------------- dense GEMM --------------------------
static LaunchDecision decide_gemm(int M, int N, int K, int lda, int ldb, int ldc, int trans_a, int trans_b, bool aligned, size_t ws_bytes,
                                  int n_cu, const PlanEnv &env) {
    const bool glds = gemm_glds_operands_ok(aligned, M, N, K, lda, ldb, trans_a, trans_b);
    if (glds && gemm_x9_wanted(M, N, K, env)) return decide_gemm_x9(M, N, K, ldc, ws_bytes, n_cu, env);
    TileRules r{};
    r.bm = (M <= 64) ? 64 : 128;
    r.allow64 = true; r.allow128 = N > 64; r.k_granule = BK;
    // (not for the [K][M] x [K][N] form -- the FC weight gradient: measured 112 vs 115 TFLOP/s)
    r.allow_bm256 = glds && (M % 256) == 0 && N > 64 && !(trans_a && trans_b);
    // (FC6 dgrad: 784 128-wide tiles = 3.06 per CU, the busiest CU carries 4 -> the plan takes another tile shape)
    const LaunchPlan plan = plan_tiles(M, N, K, r, ldc == N ? ws_bytes : 0, env);   // split-K needs ldc == N
    LaunchDecision d{};
    d.family = glds ? FAM_GLDS : FAM_STAGED;
    d.bm = plan.bm; d.bn = plan.bn;
    d.k_per_split = round_k_per_split(K, plan.splits);
    d.splits = cdiv(K, d.k_per_split);
    d.nx = cdiv(N, d.bn); d.ny = cdiv(M, d.bm);
    d.swz = 1 | (grouped_tile_order(d.nx, d.ny, M, K) ? 2 : 0);
    d.grid = d.nx * d.ny * d.splits;
    d.reduce = d.splits > 1;
    return d;
}

// A batch-1 1x1 convolution IS a dense GEMM on the NCHW tensors as they lie: Y[Cout][HW] = W[Cout][Cin] X[Cin][HW] (and its two
// gradients likewise).  The ones that are large in every dimension -- the ResNet-50 C4 detector's layer3 / RoI-head bottlenecks
// (models/mask_rcnn/resnet.py:111-148: 1024 <-> 512 <-> 2048 channels on 25088 stacked pixels) -- take the bf16 x 9 kernel.
// aligned: workspace present, both operands and the result 16-byte aligned
static bool conv1x1_takes_x9(bool aligned, int M, int N, int K, int lda, int ldb, int trans_a, int trans_b, const PlanEnv &env) {
    return gemm_glds_operands_ok(aligned, M, N, K, lda, ldb, trans_a, trans_b) && gemm_x9_wanted(M, N, K, env);
}

// ----------------------------- convolution forward / data gradient --------------------------
// GEMM view: M output rows (fwd Cout, dgrad Cin), N = batch * PH * PW pixels, K = CB * KH * KW with CB the gathered tensor's channels.
// fused_act: the data gradient's activation-gradient epilogue (no GEMM routing)
static LaunchDecision decide_conv(const ConvShape &c, bool dgrad, bool aligned, bool fused_act, size_t ws_bytes, int n_cu, const PlanEnv &env) {
    const int M = dgrad ? c.Cin : c.Cout, CB = dgrad ? c.Cout : c.Cin, PH = dgrad ? c.IH : c.OH(), PW = dgrad ? c.IW : c.OW();
    const int N = c.batch * PH * PW, K = CB * c.KH * c.KW, taps = c.KH * c.KW;
    const bool slab_aligned = (CB % BK) == 0;
    // packed weights [CB][mpad]: the GEMM's A stored [K][M]
    if (c.gemm_1x1() && slab_aligned && !fused_act && conv1x1_takes_x9(aligned, M, PH * PW, CB, conv_packed_mpad(M), PH * PW, 1, 1, env))
        return decide_gemm_x9(M, PH * PW, CB, PH * PW, ws_bytes, n_cu, env);
    LaunchDecision d{};
    if (!dgrad && c.KH == 3 && c.KW == 3 && c.S == 1 && c.P == 1 && c.Cin <= 4 && !slab_aligned && c.row_period == 0 && c.IW >= 64) {
        // image-side 3x3 layer (VGG conv1_1): direct kernel on the tap-major [Cout][9 Cin] weights the gather kernel takes
        d.family = FAM_SMALL_CIN; d.splits = 1;
        return d;
    }
    d.family = slab_aligned ? FAM_GLDS : FAM_STAGED;
    // stride-2 data gradient on the direct-to-LDS kernel: class-major N axis, a quarter of the K-slabs per tile (ConvGeom::parity)
    d.parity = c.S == 2 && dgrad && slab_aligned && (PH % 2) == 0 && (PW % 2) == 0 && taps <= 32;
    const bool small_m = M <= 64;
    TileRules r{};
    r.bm = small_m ? 64 : 128;
    r.allow64 = r.allow128 = true; r.allow256 = small_m && slab_aligned; r.k_granule = BK;
    r.allow_bm256 = slab_aligned && (M % 256) == 0;
    r.one_tap = taps == 1 && slab_aligned;
    // <= 32 output rows (the decoders' 64 -> 32 stage: 262144 pixels; the data gradient into the discriminators' 32-channel map):
    // the 32 x 256 tile, one K pass.  Taken on many pixels; SCDA_PLAN_FORCE=32,256,1 forces it wherever it is legal (tests), any
    // other forced plan keeps it out.
    r.bn32 = (M <= 32 && slab_aligned) ? 256 : 0; r.one_pass32 = true;
    // parity classes: a launch is four GEMMs of N / 4 pixels and (on average) K / 4 each
    const int planN = d.parity ? N / 4 : N, planK = d.parity ? std::max(BK, K / 4 / BK * BK) : K;
    LaunchPlan plan = plan_tiles(M, planN, planK, r, ws_bytes / (d.parity ? 4 : 1), env);
    if (r.bn32 && !env.force.set && planN >= (d.parity ? 64 * 256 : 256 * 256)) plan = LaunchPlan{256, 1, 32};
    d.bm = plan.bm; d.bn = plan.bn;
    d.k_per_split = round_k_per_split(K, plan.splits);
    d.splits = cdiv(K, d.k_per_split);
    d.nx = cdiv(N, d.bn); d.ny = cdiv(M, d.bm);
    d.swz = 1;
    if (d.parity) {
        d.nc = c.batch * (PH / 2) * (PW / 2);
        d.ncp = cdiv(d.nc, d.bn) * d.bn;
        d.nx = 4 * (d.ncp / d.bn);
        // the kernel divides each class's slabs evenly
        d.splits = fit_splits(std::max(1, std::min(plan.splits, (CB / BK) * taps)), M, N, ws_bytes);
    } else if (grouped_tile_order(d.nx, d.ny, M, K)) {
        d.swz |= 2;
    }
    d.grid = d.nx * d.ny * d.splits;
    d.reduce = d.splits > 1;
    return d;
}

// ----------------------------- convolution weight gradient --------------------------
// GEMM view: M = Cout, N = Cin * KH * KW, K = batch * OH * OW pixels; always split-K slabs + the fixed-order reduce.
// dy_aligned: dY is 16-byte aligned; aligned: ... and so are X and dW, and there is a workspace (GEMM routing);
// fused_bias: the bias gradient rides along (no GEMM routing; the caller has taken its partials' room off ws_bytes)
static LaunchDecision decide_wgrad(const ConvShape &c, bool dy_aligned, bool aligned, bool fused_bias, size_t ws_bytes, int n_cu, const PlanEnv &env) {
    const int OH = c.OH(), OW = c.OW();
    const int M = c.Cout, N = c.Cin * c.KH * c.KW, K = c.batch * OH * OW;
    // dW[Cout][Cin] (+)= dY[Cout][HW] X[Cin][HW]^T: both K-contiguous
    if (c.gemm_1x1() && !fused_bias && conv1x1_takes_x9(aligned, M, N, K, K, K, 0, 0, env)) return decide_gemm_x9(M, N, K, N, ws_bytes, n_cu, env);
    const bool small = M <= 64;
    // the LDS-DMA kernel addresses one image of dY / X through a buffer descriptor with 32-bit lane offsets
    const bool fits_2g = (long long)c.Cout * OH * OW * 4 < (1LL << 31) && (long long)c.Cin * c.IH * c.IW * 4 < (1LL << 31);
    // K-slabs of 16 pixels must not straddle two images: OH*OW % 16 == 0.  (A partial last slab for batch-1 planes was built and
    // measured: ResNet layer3's 50 x 84 weight gradients took 325 us on this kernel's general addressing path against 162 us on the
    // register-staged one -- those layers have only 4200 pixels of K to amortise the pipeline over; removed.)
    const bool glds = dy_aligned && ((OH * OW) % BK) == 0 && fits_2g;
    TileRules r{};
    r.bm = small ? 64 : 128;
    r.allow64 = N <= 64; r.allow128 = !r.allow64; r.must_split = true; r.k_granule = 32;
    r.allow_bm256 = glds && r.allow128 && (M % 256) == 0;
    // <= 32 output channels on the direct-to-LDS kernel: the 32 x 128 tile, same split count (SCDA_PLAN_FORCE=32,128,s forces it where
    // legal; any other forced plan keeps it out)
    r.bn32 = (glds && M <= 32 && r.allow128) ? 128 : 0;
    LaunchPlan plan = plan_tiles(M, N, K, r, ws_bytes, env);
    if (r.bn32 && !env.force.set) plan.bm = 32;
    LaunchDecision d{};
    d.family = glds ? FAM_GLDS : FAM_STAGED;
    d.bm = plan.bm; d.bn = plan.bn;
    d.k_per_split = (round_k_per_split(K, plan.splits) + 31) / 32 * 32;
    d.splits = cdiv(K, d.k_per_split);
    d.nx = cdiv(N, d.bn); d.ny = cdiv(M, d.bm);
    d.swz = 1;
    d.grid = d.nx * d.ny * d.splits;
    // register-staged kernel, measured: 32-deep slabs gain 10-17 % for the 64-row tiles (conv1_x, decoder heads), lose up to 8 %
    // for 128-row tiles
    d.wbk = small ? 32 : 16;
    d.reduce = 1;
    return d;
}

// ----------------------------- Winograd F(2x2, 3x3): environment, each variable read in ONE place --------------------------
// The first eight are the reference paths of the tests (tests/test_conv_wino_gpu.py and the model tests switch them between launches),
// the last two evidence aids.
struct WinoEnv {
    bool enabled;            // SCDA_WINOGRAD=0: every layer on the implicit-GEMM kernels
    bool stacked;            // SCDA_WINO_STACKED=0: ... the stacks of 7 x 7 maps
    bool pool_fuse;          // SCDA_CONV_POOL_FUSE=0: the 2x2 max-pool behind a convolution stays a launch of its own
    bool gm_set; int gm;     // SCDA_WINO_GM=2|4: that split of the XCDs over m-tile groups x pixel-block runs where legal, 0 none
    bool splits_set; int splits;               // SCDA_WINO_SPLITS: split-K count of the forward / data gradient
    bool persist;            // SCDA_WINO_PERSIST=0: one workgroup per tile also where there are more tiles than CUs
    bool wgrad_splits_set; int wgrad_splits;   // SCDA_WINO_WGRAD_SPLITS: K-split count of the weight gradient
    bool wgrad_no_groups;    // SCDA_WINO_WGRAD_NO_GROUPS: 2 or 4 splits dealt over the XCDs as they come
    int dbg;                 // SCDA_WINO_DBG: handed to conv_wino_kernel (WinoEpi::dbg: 1 no epilogue, 2 no K loop)
    const char *log;         // SCDA_WINO_LOG=<file>: one line per launch (conv_wino.hip wino_log opens and writes it)
};

// (read per call, as read_plan_env)
static WinoEnv read_wino_env() {
    const auto off = [](const char *name) { const char *v = getenv(name); return v && strcmp(v, "0") == 0; };
    const auto num = [](const char *name, bool *set) { const char *v = getenv(name); *set = v != nullptr; return v ? atoi(v) : 0; };
    WinoEnv e{};
    e.enabled = !off("SCDA_WINOGRAD");
    e.stacked = !off("SCDA_WINO_STACKED");
    e.pool_fuse = !off("SCDA_CONV_POOL_FUSE");
    e.gm = num("SCDA_WINO_GM", &e.gm_set);
    e.splits = num("SCDA_WINO_SPLITS", &e.splits_set);
    const char *pe = getenv("SCDA_WINO_PERSIST");
    e.persist = !(pe && pe[0] == '0');
    e.wgrad_splits = num("SCDA_WINO_WGRAD_SPLITS", &e.wgrad_splits_set);
    e.wgrad_no_groups = getenv("SCDA_WINO_WGRAD_NO_GROUPS") != nullptr;
    bool dbg_set;
    e.dbg = num("SCDA_WINO_DBG", &dbg_set);
    e.log = getenv("SCDA_WINO_LOG");
    return e;
}

// ----------------------------- Winograd: which convolutions take it --------------------------
constexpr int WINO_SLAB = 8;          // channels per K-slab of conv_wino_kernel (wino_pack.h)
constexpr int WINO_MIN_C = 32;        // fewer channels on either side: the implicit-GEMM kernels (the weight-gradient kernel's own floor)
constexpr int WINO_FILL_TILES = 200;  // 64-row tiles from which a launch fills the chip: below, 32-row tiles and split-K; from it, the fused pool

static bool below_2g(long long elems) { return elems * 4 < (1LL << 31); }   // (buffer descriptors with 32-bit byte offsets)

// pixel blocks of 8 x 32 output pixels, partial on the right / bottom edge (a stack of 7 x 7 maps: one block column, a block row
// per four maps)
struct WinoBlocks { int nbx, nby, npb; };
static WinoBlocks wino_blocks(int batch, int H, int W, int stack) {
    const int nbx = stack ? 1 : (W + 31) / 32, nby = stack ? (stack + 3) / 4 : (H + 7) / 8;
    return WinoBlocks{nbx, nby, batch * nby * nbx};
}
static long long wino_tiles64(int M, const WinoBlocks &b) { return (long long)((M + 63) / 64) * b.npb; }

// what conv_wino_kernel runs: y [batch, M, H, W] from x [batch, C, H, W]; stack > 0: [1, C, stack * 7, 7] as that many 7 x 7 maps
static bool wino_kernel_ok(int batch, int C, int H, int W, int M, int stack) {
    return batch > 0 && M > 0 && stack >= 0 && C >= WINO_SLAB && (C % WINO_SLAB) == 0 &&
           (stack ? batch == 1 && H == stack * 7 && W == 7 : (H % 2) == 0 && (W % 2) == 0) && below_2g((long long)C * H * W) &&
           below_2g((long long)M * H * W);
}
// ... and conv_wino_wgrad_kernel (64-channel tiles on both sides; stacked maps need whole ones)
static bool wino_wgrad_kernel_ok(int batch, int Cin, int H, int W, int Cout, int stack) {
    const int min_c = stack ? 64 : WINO_MIN_C;
    return batch > 0 && stack >= 0 && Cin >= min_c && Cout >= min_c && (stack ? batch == 1 && H == stack * 7 && W == 7 : (H % 2) == 0 && (W % 2) == 0) &&
           below_2g(64LL * H * W);
}

enum Direction { DIR_FWD = 0, DIR_DGRAD = 1, DIR_WGRAD = 2 };
enum RouteFamily { ROUTE_GEMM = 0, ROUTE_WINO = 1, ROUTE_WINO_STACKED = 2 };
struct ConvRoute {
    int family;
    int maps;       // the image is a stack of this many 7 x 7 maps (row period 7: the ResNet-50 C4 detector's channel-major RoI head), else 0
    bool pool;      // forward: conv + activation + 2x2 max-pool may run as ONE Winograd launch (the fused epilogue needs finished values:
                    // a launch that fills the chip without split-K)
};

// c as the entry points receive it (Cin / Cout of the FORWARD convolution, IH x IW its input): stride-1 pad-1 3x3 layers the kernels
// can run, from WINO_MIN_C channels a side
static ConvRoute route_conv(int dir, const ConvShape &c, const WinoEnv &env) {
    ConvRoute r{ROUTE_GEMM, 0, false};
    if (c.row_period == 7 && c.IW == 7 && c.batch == 1 && c.IH % 7 == 0 && env.stacked) r.maps = c.IH / 7;
    if (!(env.enabled && c.KH == 3 && c.KW == 3 && c.S == 1 && c.P == 1) || (c.row_period && !r.maps)) return r;
    const int C = dir == DIR_DGRAD ? c.Cout : c.Cin, M = dir == DIR_DGRAD ? c.Cin : c.Cout;   // the data gradient reduces over Cout
    if (dir == DIR_WGRAD ? !wino_wgrad_kernel_ok(c.batch, c.Cin, c.IH, c.IW, c.Cout, r.maps)
                         : !(std::min(C, M) >= WINO_MIN_C && wino_kernel_ok(c.batch, C, c.IH, c.IW, M, r.maps)))
        return r;
    r.family = r.maps ? ROUTE_WINO_STACKED : ROUTE_WINO;
    r.pool = dir == DIR_FWD && !r.maps && env.pool_fuse && wino_tiles64(M, wino_blocks(c.batch, c.IH, c.IW, 0)) >= WINO_FILL_TILES;
    return r;
}

// ----------------------------- Winograd forward / data gradient --------------------------
enum WinoEpilogue { WINO_EPI_PLAIN = 0, WINO_EPI_MASK = 1, WINO_EPI_POOL = 2, WINO_EPI_SPLIT = 3 };   // conv_wino_kernel's EPI

struct WinoDecision {
    int mb;               // tile rows / 32
    int pixel_major;      // XCD order: contiguous pixel-block runs per XCD (else m-tile-major)
    int gm;               // the 8 XCDs split gm x (8 / gm) over m-tile groups x pixel-block runs (1: no split)
    int splits, slabs_per_split;
    int per_xcd;          // pixel_major: (split, pixel block) items per XCD
    int n_wg;             // workgroup slots of the launch: the grid of the one-tile-per-workgroup form
    int persist;          // one workgroup per CU walks the tiles (grid = n_cu)
    int epi;
};

// y [batch, M, H, W]; pool: the fused 2x2 max-pool, masked: the producer's activation mask (data gradient)
static WinoDecision decide_wino(int batch, int C, int H, int W, int M, int stack, bool pool, bool masked, size_t ws_bytes, int n_cu,
                                const WinoEnv &env) {
    WinoDecision d{};
    // tile rows: 64 (every fragment feeds two MFMAs), or 32 for layers with <= 32 output rows (the decoders' 64 -> 32 stage: half of
    // a 64-row tile would multiply padding).  Measured on every VGG / decoder layer (scripts/bench_wino.py): the two are within 3 % of
    // each other everywhere else -- two co-resident 32-row workgroups start and finish together, so one's start-up and epilogue do
    // NOT hide under the other's K loop.
    // ... and for launches that would not fill the chip with 64-row tiles (the decoders' batch-4 residual convolutions: 128 tiles;
    // conv5_x / the RPN: 64): twice the workgroups first, split-K (slabs + a reduce launch) only for what is still missing
    const WinoBlocks blocks = wino_blocks(batch, H, W, stack);
    const int npb = blocks.npb;
    d.mb = (M <= 32 || wino_tiles64(M, blocks) < WINO_FILL_TILES) ? 1 : 2;
    const int n_mbg = (M + 63) / 64 * 2, n_mt = (M + 32 * d.mb - 1) / (32 * d.mb), n_slab = C / WINO_SLAB;
    // XCD order: pixel-block-major when all m-tiles' filters can stream through one XCD's 4 MB L2 beside the patches (<= 4.5 MB: every
    // layer below 512 output channels; conv3_2's 4.2 MB: 290 -> 109 MB read per launch), m-tile-major otherwise.  ALSO with a single
    // m-tile (conv1_2, the decoders' up-sampling stages): dealt round-robin, row neighbours run on different XCDs and each fetches the
    // two extra 128-byte lines its 136-byte patch rows straddle -- conv1_2 read 422 MB for a 134 MB input, 183 MB as contiguous runs
    // (and the decoders' stages run 4 - 9 % faster).
    // (... and only for launches of >= 16 pixel blocks per XCD: the runs leave up to 7 idle workgroups per m-tile, and a small
    // launch -- the decoders' 64 blocks -- lost 13 % to the imbalance)
    const double u_bytes = 16.0 * n_mbg * 32 * C * 4, in_bytes = 4.0 * batch * C * H * W;
    d.pixel_major = npb >= 128 && u_bytes <= 4.5e6;
    // filters beyond one L2: split the XCDs gm x (8 / gm) over m-tile groups x pixel-block runs where that moves fewer bytes than
    // m-tile-major (filters x (8 / gm) + input x gm against filters + input x min(n_mt, 8)) and every XCD still streams <= 4.5 MB
    // of filters
    d.gm = 1;
    if (!d.pixel_major) {
        const int gm_legacy = n_mt >= 8 ? 8 : n_mt;
        // (fewer than 8 m-tiles: a block's row neighbours land on different XCDs and each fetches the straddled lines itself)
        double best = u_bytes * (8.0 / gm_legacy) + in_bytes * gm_legacy * (n_mt >= 8 ? 1.0 : 2.0);
        for (int c = 2; c <= 4; c *= 2) {
            const long long items = (long long)npb;     // (the split count is not known yet: launches that split are small, see below)
            if (n_mt % c != 0 || items % (8 / c) != 0 || items / (8 / c) < 8 || u_bytes / c > 4.5e6) continue;
            const double cost = u_bytes * (8.0 / c) + in_bytes * c;
            if (env.gm_set ? env.gm == c : cost < best) { best = cost; d.gm = c; }
        }
        if (env.gm_set && env.gm == 0) d.gm = 1;
        if (d.gm > 1) d.pixel_major = 1;
    }
    // split-K: a launch below one workgroup per CU splits the channel loop (>= 4 slabs per split), slabs in the natural pixel order
    // (two 32-row workgroups per CU: conv5_x 65 -> 61 us; 32-row tiles at one per CU: the decoders' 256-tile launches run 10 % faster
    // unsplit, and without a reduce launch)
    const long long tiles = (long long)n_mt * npb;
    const size_t out_bytes = (size_t)M * batch * H * W * sizeof(float);
    int splits = 1;
    if (env.splits_set) splits = env.splits;
    else if (tiles < WINO_FILL_TILES) splits = (int)std::min<long long>((256 * (3 - d.mb) + tiles / 2) / tiles, n_slab / 4 > 0 ? n_slab / 4 : 1);
    if (splits < 1) splits = 1;
    while (splits > 1 && (size_t)splits * out_bytes > ws_bytes) --splits;
    if (pool) splits = 1;      // (the fused pool needs finished values in the epilogue; its callers are the 256+-tile VGG layers)
    if (out_bytes >= ((size_t)1 << 31)) splits = 1;      // (a slab is addressed with 32-bit byte offsets)
    d.slabs_per_split = (n_slab + splits - 1) / splits;
    d.splits = (n_slab + d.slabs_per_split - 1) / d.slabs_per_split;
    long long wgs = tiles * d.splits;
    if (d.pixel_major) {      // 8 / gm runs of per_xcd (split, pixel block) items x n_mt m-tiles; the last run may hold idle workgroups
        const int gp = 8 / d.gm;
        d.per_xcd = (int)(((long long)npb * d.splits + gp - 1) / gp);
        wgs = 8LL * d.per_xcd * (n_mt / d.gm);
    }
    d.n_wg = (int)wgs;
    // more 64-row tiles than CUs: one persistent workgroup per CU walks them (see the kernel)
    // (a split launch is never persistent: the automatic heuristic only splits launches below one workgroup per CU, but
    //  SCDA_WINO_SPLITS can force one where there are more -- the split-slab epilogue exists in the one-tile form only)
    d.persist = d.mb == 2 && d.splits == 1 && wgs > n_cu && d.slabs_per_split >= 2 && n_slab >= 2 && env.persist && out_bytes < ((size_t)1 << 31);
    d.epi = d.splits > 1 ? WINO_EPI_SPLIT : pool ? WINO_EPI_POOL : masked ? WINO_EPI_MASK : WINO_EPI_PLAIN;
    return d;
}

// ----------------------------- Winograd weight gradient --------------------------
struct WinoWgradDecision {
    int n_slab;           // K-slabs of the launch: 2 x 16 pixels each (stacked maps: one tile row of a pair of maps)
    int splits, slabs_per_split;
    int splits_per_xcd;   // splits % 8 == 0: whole runs of splits per XCD (else 0)
    int order;            // 0 workgroups dealt over the XCDs as they come, 1 whole splits per XCD, 2 one split + one m-tile group per XCD
    int grid;
};

// dw [Cout, Cin, 3, 3]; with_db: 1024 rows of bias-gradient partials share the workspace
static WinoWgradDecision decide_wino_wgrad(int batch, int Cin, int H, int W, int Cout, int stack, bool with_db, size_t ws_bytes,
                                           const WinoEnv &env) {
    WinoWgradDecision d{};
    const int n_mt = (Cout + 63) / 64, n_ct = (Cin + 63) / 64;
    d.n_slab = stack ? (stack + 1) / 2 * 4 : batch * (H / 2) * ((W + 15) / 16);
    const long long tiles = (long long)n_mt * n_ct;
    const size_t slab_bytes = (size_t)Cout * Cin * 9 * sizeof(float), db_bytes = with_db ? (size_t)1024 * Cout * sizeof(float) : 0;
    // one workgroup per CU and round: splits so that the launch has ~256 workgroups (>= 8 slabs each, <= 1024 splits)
    int splits = env.wgrad_splits_set ? env.wgrad_splits : (int)((256 + tiles - 1) / tiles);
    splits = std::max(1, std::min(std::min(splits, 1024), std::max(1, d.n_slab / 8)));
    if (splits >= 8) splits = (splits + 7) / 8 * 8;      // whole runs per XCD (the last XCD's run would otherwise hold idle workgroups)
    splits = std::min(splits, std::max(1, d.n_slab / 4));
    while (splits > 1 && (size_t)splits * slab_bytes + db_bytes > ws_bytes) --splits;
    d.slabs_per_split = (d.n_slab + splits - 1) / splits;
    d.splits = (d.n_slab + d.slabs_per_split - 1) / d.slabs_per_split;
    d.splits_per_xcd = (d.splits % 8) == 0 ? d.splits / 8 : 0;
    const bool groups = !env.wgrad_no_groups && (d.splits == 2 || d.splits == 4) && n_mt % (8 / d.splits) == 0;
    d.order = d.splits_per_xcd > 0 ? 1 : groups ? 2 : 0;
    d.grid = (int)(tiles * d.splits);
    return d;
}

}  // namespace lp
}  // namespace scda

#endif
