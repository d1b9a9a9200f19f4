"""numpy statement of the cluster-region rule (include/scda_ops.h, scda_kmeans_hip): sklearn 1.7.2's
KMeans(n_clusters=k, random_state=0).fit on the RoI centres (k-means++ seeding, one Lloyd run), then the member rows of
functions/mask.py:214-230.  The second statement that the kernels and the fixtures of tests/golden/kmeans_ref.npz are both
compared with.  Arithmetic: float64 on the float32 centred points, direct squared distances, every sum in the fixed order `sum64`
states (the kernel's), so that this file and the kernel agree bit for bit and not merely within a tolerance."""
import math

import numpy as np

CAPACITY = 1024     # points
MAX_K = 8
MAX_ITER = 300
TOL = 1e-4

_SEEDING = {}


def seeding_constants(N, k):
    """-> (first seed index, uniforms float64 [k-1, t]): the draws _kmeans_plusplus takes from np.random.RandomState(0), which KMeans
    re-creates on every fit: `choice(N, p=1/N)` = one random_sample() looked up in the normalised float64 cumsum of p (side='right'),
    then t = 2 + int(ln k) uniforms per further centre.  They depend on (N, k) only."""
    hit = _SEEDING.get((N, k))
    if hit is None:
        rs = np.random.RandomState(0)
        t = 2 + int(math.log(k))
        p = np.full(N, 1.0 / N)
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        first = int(np.searchsorted(cdf, rs.random_sample(), side='right'))
        u = np.array([rs.random_sample(t) for _ in range(k - 1)], dtype=np.float64).reshape(k - 1, t)
        hit = _SEEDING[(N, k)] = (first, u)
    return hit


def sum64(v):
    """float64 sum of v in the kernel's order: lane l of 64 adds v[l], v[l+64], ... in turn (starting from 0.0), then the 64 partial
    sums meet in a butterfly (lane l adds lane l^32's value, then l^16, ... l^1)"""
    v = np.asarray(v, dtype=np.float64)
    pad = (-v.shape[0]) % 64
    lanes = np.concatenate([v, np.zeros(pad)]).reshape(-1, 64).cumsum(axis=0)[-1] if v.shape[0] else np.zeros(64)
    ix = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[ix ^ s]
    return float(lanes[0])


def roi_centres(rois):
    """RoI rows (b, x1, y1, x2, y2, ...) -> float32 [N,2] (functions/mask.py:183-191 on float32 rows)"""
    r = np.asarray(rois, dtype=np.float32)
    return np.stack([(r[:, 3] + r[:, 1]) / np.float32(2.0), (r[:, 4] + r[:, 2]) / np.float32(2.0)], axis=1)


def _sqdist(x, y, cx, cy):
    dx, dy = x - cx, y - cy
    return dx * dx + dy * dy


def _assign(x, y, centres):
    d = np.stack([_sqdist(x, y, cx, cy) for cx, cy in centres], axis=0)
    return np.argmin(d, axis=0).astype(np.int32)          # the first minimum


def kmeans(rois, k, first=None, uniforms=None):
    """-> dict(centres float32 [k,2], labels int32 [N], counts int32 [k], seed_index int32 [k], n_iter, status); status bit 0: a cluster
    went empty (sklearn would relocate it: not restated, the other outputs are then unspecified), bit 1: bad arguments / over capacity,
    bit 2: a mean or the tolerance is not finite (a NaN or infinite point, on which sklearn raises)"""
    X = roi_centres(rois)
    N = X.shape[0]
    if not (1 <= k <= MAX_K and k <= N <= CAPACITY):
        return {"status": 2}
    if first is None:
        first, uniforms = seeding_constants(N, k)
    Xd = X.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean64 = np.array([sum64(Xd[:, 0]) / N, sum64(Xd[:, 1]) / N])
        d0, d1 = Xd[:, 0] - mean64[0], Xd[:, 1] - mean64[1]
        tol_abs = TOL * ((sum64(d0 * d0) / N + sum64(d1 * d1) / N) / 2.0)
    if not (np.isfinite(mean64).all() and np.isfinite(tol_abs)):
        return {"status": 4}                               # a NaN or infinite point: sklearn raises, the host path answers
    mean32 = mean64.astype(np.float32)
    Xc = (X - mean32[None, :]).astype(np.float64)          # float32 subtraction, as sklearn centres float32 data
    x, y = Xc[:, 0], Xc[:, 1]
    # k-means++ (_kmeans_plusplus)
    seeds = [first]
    closest = _sqdist(x, y, x[first], y[first])
    pot = sum64(closest)
    for c in range(1, k):
        cum = np.cumsum(closest)                           # sequential, float64 (stable_cumsum)
        cand = np.minimum(np.searchsorted(cum, uniforms[c - 1] * pot), N - 1)
        trial = [np.minimum(closest, _sqdist(x, y, x[j], y[j])) for j in cand]
        pots = [sum64(t) for t in trial]
        best = int(np.argmin(pots))                        # the first minimum
        closest, pot = trial[best], pots[best]
        seeds.append(int(cand[best]))
    centres = [(x[s], y[s]) for s in seeds]
    # Lloyd
    old = np.full(N, -1, dtype=np.int32)
    status, n_iter, rerun = 0, MAX_ITER, True
    for it in range(MAX_ITER):
        labels = _assign(x, y, centres)
        counts = np.bincount(labels, minlength=k)
        if (counts == 0).any():
            return {"status": 1}
        new = [(sum64(np.where(labels == c, x, 0.0)) / counts[c], sum64(np.where(labels == c, y, 0.0)) / counts[c]) for c in range(k)]
        shift = 0.0
        for (ax, ay), (bx, by) in zip(centres, new):
            shift = shift + _sqdist(bx, by, ax, ay)
        centres = new
        if np.array_equal(labels, old):
            n_iter, rerun = it + 1, False                  # strict convergence: the means just computed, no further E-step
            break
        if shift <= tol_abs:
            n_iter = it + 1
            break
        old = labels
    if rerun:
        labels = _assign(x, y, centres)
        counts = np.bincount(labels, minlength=k)
        if (counts == 0).any():
            status = 1                                     # finally empty: the reference raises; the host path does that
    c32 = np.array(centres, dtype=np.float64).astype(np.float32) + mean32[None, :]
    return {"centres": c32.astype(np.float32), "labels": labels, "counts": counts.astype(np.int32),
            "seed_index": np.array(seeds, dtype=np.int32), "n_iter": n_iter, "status": status}


def member_rows(labels, k, threshold):
    """functions/mask.py:214-230: per cluster its RoI indices ascending, the first `threshold` of them, or a with-replacement resample
    from numpy's GLOBAL generator when there are fewer -> int64 [k, threshold]"""
    rows = []
    for c in range(k):
        member = np.where(labels == c)[0]
        if member.shape[0] < threshold:
            member = member[np.random.choice(member.shape[0], threshold, replace=True)]
        else:
            member = member[0:threshold]
        rows.append(member)
    return np.stack(rows, axis=0).astype(np.int64)


def cluster_rows(rois, k, threshold):
    """steps 1-7 -> (rows int64 [k, threshold], centres float32 [k,2], the k-means dict), or (None, None, dict) when status != 0"""
    km = kmeans(rois, k)
    if km["status"]:
        return None, None, km
    return member_rows(km["labels"], k, threshold), km["centres"], km
