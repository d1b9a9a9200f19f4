"""Edge cases for the k-means kernel (scda_amd/csrc/cluster_ops.hip: kmeans_kernel), as data builders: the smallest shapes at which
each of its mechanisms can go wrong.  Seeded np.random.RandomState only.  `cases()` -> a list of (name, class, rois float32 [N, 5],
k, threshold); the rows are (b, x1, y1, x2, y2) boxes in a 1024 x 512 image, as in tests/golden/make_golden_kmeans.py.

class      what it reaches in the kernel
wave       N = 1 / 2 / 5, a wave's 63 / 64 / 65, two waves' 127 / 128 / 129 and the cap's 1023 / 1024 points: the strided sums' last
           trip, the ballot compaction's partial last wave, the binary search's clip to N - 1; k = 1 (no seeding round, no draws) up
           to k = 8 (all sixteen M-step waves)
n_eq_k     every point its own cluster: counts of one, means equal to the points
lattice    centres on an integer-pitch grid: exactly equidistant points (the E-step's first minimum) and exactly equal trial
           potentials (the seeding's first minimum)
collinear  one axis without variance
coincident one point 70 times, k = 1: tolerance 0 and shift 0
clumps     two tight clumps far apart: k = 4 splits sub-pixel clouds
duplicates exactly k distinct points padded to 200 rows: zero potential once every distinct point is a seed
halfpixel  unit boxes on a half-integer grid: the float32 centring is exact and near-ties abound
fallback   fewer than k distinct points: a cluster goes empty (status bit 0), nothing else is specified"""
import numpy as np

W, H = 1024, 512
WAVE_N = (1, 2, 5, 63, 64, 65, 127, 128, 129, 1023, 1024)
KS = (1, 2, 4, 8)


def boxes(cx, cy, w, h):
    cx, cy, w, h = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(cx, cy, w, h))
    x1, y1 = np.clip(cx - w / 2, 0, W - 1), np.clip(cy - h / 2, 0, H - 1)
    x2, y2 = np.clip(cx + w / 2, 0, W - 1), np.clip(cy + h / 2, 0, H - 1)
    return np.stack([np.zeros_like(x1), x1, y1, x2, y2], axis=1).astype(np.float32)


def uniform(seed, n):
    r = np.random.RandomState(seed)
    return boxes(r.uniform(0, W, n), r.uniform(0, H, n), np.exp(r.uniform(np.log(8), np.log(400), n)), np.exp(r.uniform(np.log(8), np.log(300), n)))


def lattice(side, pitch, x0, y0):
    """side x side box centres at an integer pitch, 4 x 4 boxes (so that x1 + x2 and y1 + y2 are exact), row-major"""
    iy, ix = np.divmod(np.arange(side * side), side)
    return boxes(x0 + pitch * ix, y0 + pitch * iy, 4.0, 4.0)


def cases():
    out = []
    for n in WAVE_N:
        for rep in range(3 if n < 1000 else 1):
            rois = uniform(10000 + 10 * n + rep, n)
            for k in KS:
                if k <= n:
                    out.append(("wave_%d_%d_s%d" % (n, k, rep), "wave", rois, k, 64))
    for k in (2, 4, 8):
        out.append(("n_eq_k_%d" % k, "n_eq_k", uniform(20000 + k, k), k, 128))
    for side, pitch, x0, y0 in ((8, 16, 400.0, 200.0), (32, 8, 300.0, 100.0)):
        for k in (2, 4, 8):
            out.append(("lattice_%dx%d_%d" % (side, side, k), "lattice", lattice(side, pitch, x0, y0), k, 16))
    r = np.random.RandomState(30000)
    line = boxes(r.uniform(40, W - 40, 100), 256.0, 16.0, 16.0)
    for k in (2, 4):
        out.append(("collinear_%d" % k, "collinear", line, k, 32))
    out.append(("coincident_70_1", "coincident", boxes(np.full(70, 333.0), np.full(70, 222.0), 20.0, 10.0), 1, 64))
    r = np.random.RandomState(30001)
    cx = np.concatenate([12.0 + r.normal(0, 0.5, 300), 1011.0 + r.normal(0, 0.5, 300)])
    clumps = boxes(cx, 250.0 + r.normal(0, 0.5, 600), 16.0, 16.0)
    for k in (2, 4):
        out.append(("clumps_%d" % k, "clumps", clumps, k, 128))
    for k in (2, 4, 8):
        r = np.random.RandomState(30010 + k)
        base = uniform(30020 + k, k)
        rows = base[np.concatenate([np.arange(k), r.randint(0, k, 200 - k)])]
        out.append(("duplicates_%d" % k, "duplicates", rows, k, 32))
    r = np.random.RandomState(30030)
    out.append(("halfpixel_500_4", "halfpixel", boxes(r.randint(2, 2 * W - 2, 500) / 2.0, r.randint(2, 2 * H - 2, 500) / 2.0, 1.0, 1.0), 4, 128))
    return out


def fallback_cases():
    """fewer than k distinct points at N = 2, 65 and 1024 -> (name, 'fallback', rois, k, threshold)"""
    out = []
    for j, (n, k, distinct) in enumerate(((2, 2, 1), (65, 4, 3), (1024, 8, 5))):
        r = np.random.RandomState(30040 + j)
        base = uniform(30050 + j, distinct)
        rows = base[np.concatenate([np.arange(distinct), r.randint(0, distinct, n - distinct)])]
        out.append(("fallback_%d_%d_%d" % (n, k, distinct), "fallback", rows, k, 32))
    return out


def case(name):
    """one case by name (the GPU tests use a few outside the fixture loop)"""
    for c in cases() + fallback_cases():
        if c[0] == name:
            return c
    raise KeyError(name)
