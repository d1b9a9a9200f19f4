// soft_nms.hip -- soft-NMS (extensions/_cython_bbox/cython_nms.pyx:98-203: hard, linear and Gaussian rescoring) of S independent
// lists in one launch, bit for bit: the surviving rows, their order and their final scores.
//
// One wave64 per list.  The reference is a chain of n dependent outer iterations (pick the best live row, rescore every live row it
// overlaps, discard what fell below the threshold); an iteration is at most a few hundred rows wide, so depth decides the time and a
// single wave pays no workgroup barrier for it: kSoftWave threads per workgroup make __syncthreads() a wave-local ordering point.
// The lists of a batch run side by side, one per workgroup.
//
// The working copy of a list -- x1, y1, x2, y2, score, original index -- lives in LDS (6 x 2048 x 4 bytes = 48 KB) with two short
// scratch lists for the compaction (4 KB).  One iteration i on the live range [i, N):
//   1. m = the first position of [i, N) with the largest score (the reference updates on strict <: the lowest position wins a tie);
//      entries i and m are swapped; t = entry i.  Non-finite scores follow the reference's `maxscore < boxes[pos, 4]` from
//      maxscore = boxes[i, 4]: a NaN AT i is selected (nothing is greater than it), a NaN anywhere else is never greater; +-inf order
//      as numbers.  m is the same in every lane whatever the scores hold.
//   2. every pos in (i, N) in parallel: the IoU(+1) with t in the reference's arithmetic -- Cython writes the source's "+ 1" beside
//      a C float as "+ 1.0", so those sums and the products around them are evaluated in double and rounded once where they are
//      assigned to a `cdef float`; iw * ih and the division are float32.  Only a row with iw > 0 and ih > 0 is touched at all: one
//      that does not overlap t is neither rescored nor discarded, whatever its score.
//   3. weight: hard (ov > Nt ? 0 : 1), linear (ov > Nt ? 1 - ov : 1) or Gaussian ((float)exp((double)(-(ov * ov) / sigma)), the
//      argument formed in float32, exp the double routine); score = weight * score in float32; dead when score < threshold.
//   4. the reference discards a dead row by copying the LAST live row over it, shrinking N and examining that place again.  With
//      S survivors in (i, N) and N' = i + 1 + S that is: the k-th lowest dead position below N' receives the k-th HIGHEST survivor
//      at or above N' (there are equally many of both), survivors below N' stay, N = N'.  The order matters only for which of
//      several equal scores is "first" later on.
// After the last iteration positions [0, N) are the selections in order.  Every loop is bounded by the list length (i < N, and N
// never grows); no atomics, no spinning; two runs write the same bytes.
#include <math.h>

#include "common.h"

namespace scda {

constexpr int kSoftCap = 2048;     // rows of one list (the six working arrays fill 48 KB of LDS)
constexpr int kSoftWave = kWave;   // ONE wave per list: see wave_sync
constexpr unsigned kDeadBit = 0x80000000u;

// Orders the LDS traffic of the one wave of the workgroup: a workgroup that fits a wave needs no hardware barrier (the compiler
// lowers this one to a wave barrier with the LDS fence), but what other lanes wrote must be visible before it is read.
__device__ __forceinline__ void wave_sync() { __syncthreads(); }

__global__ __launch_bounds__(kSoftWave) void soft_nms_segments_kernel(float *__restrict__ boxes, const long long *__restrict__ seg,
                                                                      const int max_n, const int method, const float sigma,
                                                                      const float Nt, const float threshold,
                                                                      long long *__restrict__ keep, long long *__restrict__ num_out) {
    __shared__ float sx1[kSoftCap], sy1[kSoftCap], sx2[kSoftCap], sy2[kSoftCap], ssc[kSoftCap];
    __shared__ unsigned sid[kSoftCap];                                  // original row | kDeadBit while a row waits for its compaction
    __shared__ unsigned short dlist[kSoftCap / 2], slist[kSoftCap / 2];  // dead places below N' / survivors at or above it, ascending
    const int s = blockIdx.x, lane = threadIdx.x;
    const long long first = seg[3 * (size_t)s];
    const long long len = seg[3 * (size_t)s + 1];
    const int n = (int)(len < 0 ? 0 : len > (long long)min(max_n, kSoftCap) ? (long long)min(max_n, kSoftCap) : len);
    float *rows = boxes + (size_t)first * 5;
    for (int p = lane; p < n; p += kSoftWave) {
        const float *r = rows + (size_t)p * 5;
        sx1[p] = r[0]; sy1[p] = r[1]; sx2[p] = r[2]; sy2[p] = r[3]; ssc[p] = r[4];
        sid[p] = (unsigned)p;
    }
    wave_sync();
    const unsigned long long below = (1ull << lane) - 1ull;             // the lanes before this one
    int N = n;
    for (int i = 0; i < N; ++i) {
        // ---- 1. the first maximum of [i, N)
        constexpr int kNone = 0x7fffffff;
        const float s0 = ssc[i];                                        // (one address: the same value in every lane)
        float bs = 0.f;
        int bp = kNone;
        for (int p = i + lane; p < N; p += kSoftWave) {
            const float v = ssc[p];
            if (v == v && (bp == kNone || v > bs)) { bs = v; bp = p; }  // ascending p per lane: strict > keeps the lowest position
        }
        // a NaN is never a candidate, so the (bs, bp) pairs are totally ordered and the butterfly leaves ONE pair in all lanes
#pragma unroll
        for (int off = 1; off < kSoftWave; off <<= 1) {
            const float os = __shfl_xor(bs, off, kSoftWave);
            const int op = __shfl_xor(bp, off, kSoftWave);
            if (op != kNone && (bp == kNone || os > bs || (os == bs && op < bp))) { bs = os; bp = op; }
        }
        // a NaN at i is its own maximum (`NaN < v` never holds); otherwise place i is a candidate and bp is in [i, N) (clamp: a guard)
        const int m = s0 != s0 ? i : min(max(bp, i), N - 1);
        const float tx1 = sx1[m], ty1 = sy1[m], tx2 = sx2[m], ty2 = sy2[m], ts = ssc[m];
        const unsigned tid_ = sid[m];
        wave_sync();                                                    // every lane holds t before lane 0 overwrites place m
        if (lane == 0 && m != i) {
            sx1[m] = sx1[i]; sy1[m] = sy1[i]; sx2[m] = sx2[i]; sy2[m] = sy2[i]; ssc[m] = ssc[i]; sid[m] = sid[i];
            sx1[i] = tx1; sy1[i] = ty1; sx2[i] = tx2; sy2[i] = ty2; ssc[i] = ts; sid[i] = tid_;
        }
        wave_sync();
        // ---- 2. + 3. rescore (i, N); count the dead
        const double tarea = ((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0);
        int n_dead = 0;
        for (int base = i + 1; base < N; base += kSoftWave) {
            const int p = base + lane;
            bool dead = false;
            if (p < N) {
                const float x1 = sx1[p], y1 = sy1[p], x2 = sx2[p], y2 = sy2[p];
                // the reference's own min / max (cython_nms.pyx:28-32: `a if a <= b else b`, t's coordinate first): a NaN in t's
                // coordinate gives the row's, a NaN in the row's is returned (fminf / fmaxf would drop it) and the row is not touched
                const float iw = (float)((double)((tx2 <= x2 ? tx2 : x2) - (tx1 >= x1 ? tx1 : x1)) + 1.0);
                const float ih = (float)((double)((ty2 <= y2 ? ty2 : y2) - (ty1 >= y1 ? ty1 : y1)) + 1.0);
                if (iw > 0.f && ih > 0.f) {
                    const float area = (float)(((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0));
                    const float inter = iw * ih;
                    const float ua = (float)(tarea + (double)area - (double)inter);
                    const float ov = inter / ua;
                    float weight;
                    if (method == 1) weight = ov > Nt ? 1.f - ov : 1.f;
                    else if (method == 2) weight = (float)exp((double)(-(ov * ov) / sigma));
                    else weight = ov > Nt ? 0.f : 1.f;
                    const float sc = weight * ssc[p];
                    ssc[p] = sc;
                    dead = sc < threshold;
                    if (dead) sid[p] |= kDeadBit;
                }
            }
            n_dead += __popcll(__ballot(dead));
        }
        wave_sync();
        if (n_dead == 0) continue;                                      // (uniform over the wave)
        // ---- 4. compaction: N' = N - n_dead
        const int Nn = N - n_dead;
        int n_lo = 0, n_hi = 0;                                         // dead places below N', survivors at or above it, so far
        for (int base = i + 1; base < N; base += kSoftWave) {
            const int p = base + lane;
            const bool dead = p < N && (sid[p] & kDeadBit);
            const bool lo = dead && p < Nn, hi = p < N && !dead && p >= Nn;
            const unsigned long long blo = __ballot(lo), bhi = __ballot(hi);
            if (lo) dlist[n_lo + __popcll(blo & below)] = (unsigned short)p;
            if (hi) slist[n_hi + __popcll(bhi & below)] = (unsigned short)p;
            n_lo += __popcll(blo);
            n_hi += __popcll(bhi);
        }
        wave_sync();
        const int moves = min(n_lo, n_hi);                              // (equal; min: a guard)
        for (int k = lane; k < moves; k += kSoftWave) {
            const int dst = dlist[k], src = slist[n_hi - 1 - k];        // sources lie at or above N', destinations below: disjoint
            sx1[dst] = sx1[src]; sy1[dst] = sy1[src]; sx2[dst] = sx2[src]; sy2[dst] = sy2[src]; ssc[dst] = ssc[src]; sid[dst] = sid[src];
        }
        N = Nn;
        wave_sync();
    }
    wave_sync();
    for (int p = lane; p < N; p += kSoftWave) {
        const unsigned r = sid[p] & ~kDeadBit;
        keep[first + p] = (long long)r;
        rows[(size_t)r * 5 + 4] = ssc[p];
    }
    if (lane == 0) num_out[s] = N;
}

}  // namespace scda

using namespace scda;

SCDA_API int scda_soft_nms_capacity(void) { return kSoftCap; }

SCDA_API int scda_soft_nms_segments_hip(float *boxes, const long long *seg, int S, int max_n, int method, float sigma, float Nt,
                                        float threshold, int64_t *keep, int64_t *num_out, void *stream) {
    if (S <= 0 || S > 0x7fffffff / 3 || max_n < 0 || max_n > kSoftCap || method < 0 || method > 2 || !seg || !num_out ||
        (max_n > 0 && (!boxes || !keep))) {
        set_error("scda_soft_nms_segments_hip: bad arguments (S %d, max_n %d of at most %d, method %d)", S, max_n, kSoftCap, method);
        return SCDA_EINVAL;
    }
    hipLaunchKernelGGL(soft_nms_segments_kernel, dim3(S), dim3(kSoftWave), 0, as_stream(stream), boxes, seg, max_n, method, sigma, Nt,
                       threshold, (long long *)keep, (long long *)num_out);
    return launch_status("soft_nms_segments_kernel");
}
