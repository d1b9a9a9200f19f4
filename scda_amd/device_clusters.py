"""Cluster-region generator on the device: the k-means over the RoI centres and the gather of the cluster
features on the MI355X (scda_amd/csrc/cluster_ops.hip), replacing sklearn's KMeans(n_clusters, random_state=0).fit on the host
and ATen's index_select of functions/mask.py:193-237.

The rule restated is scikit-learn 1.7.2's (include/scda_ops.h states it); the device path does not depend on the scikit-learn the
process would import.  Its k-means++ draws come from a RandomState(0) that KMeans re-creates on every fit, so they are constants
of (N, k): drawn once here, cached, handed to the kernel as arguments.

What stays on the host, because it IS the reference's observable behaviour: the np.random.choice draws from numpy's GLOBAL
generator for clusters smaller than `threshold` (:218-220), in the reference's order; the device sends back the k counts, the k
centres and a status word (under 100 bytes, one pinned buffer, one short synchronise of the box logic's side stream), the host
draws and uploads the picks, and the gather is enqueued on the compute stream behind the features.  Nothing else waits.

What is not covered: sklearn's relocation of a cluster that goes empty during Lloyd (the kernel raises a status flag), a NaN or infinite
RoI coordinate (sklearn raises a ValueError on it; the kernel raises another flag so that the host path does), more than
scda_kmeans_capacity() = 1024 points, more than 8 clusters, features that are not float32 rows on the device.  All of these take
the unchanged sklearn path for that call, on the same state of the global generator.

`enabled()` is the switch: SCDA_DEVICE_KMEANS=1 turns the device path on; the default is off."""
import ctypes
import logging
import math
import os

import numpy as np
import torch

from scda_amd import native as N
from scda_amd.dropin import backend

MAX_K = 8
_SEEDING = {}
_PINNED = {}
logger = logging.getLogger(__name__)


def enabled():
    return os.environ.get("SCDA_DEVICE_KMEANS", "0") == "1" and torch.cuda.is_available()


def seeding_constants(n, k):
    """-> (first seed index, ctypes double [(k-1) * t] or None, t): what _kmeans_plusplus draws from np.random.RandomState(0) for n
    points and k clusters -- `choice(n, p=1/n)` (one random_sample() looked up in the normalised float64 cumsum of p, side='right'),
    then t = 2 + int(ln k) uniforms per further centre"""
    hit = _SEEDING.get((n, k))
    if hit is None:
        rs = np.random.RandomState(0)
        t = 2 + int(math.log(k))
        cdf = np.cumsum(np.full(n, 1.0 / n))
        cdf /= cdf[-1]
        first = int(np.searchsorted(cdf, rs.random_sample(), side='right'))
        u = np.concatenate([rs.random_sample(t) for _ in range(k - 1)]) if k > 1 else None
        hit = _SEEDING[(n, k)] = (first, None if u is None else (ctypes.c_double * u.size)(*u.tolist()), t)
    return hit


def _covered(rois, features, k, threshold):
    if not (torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32 and features.dim() == 2
            and features.stride(1) == 1 and features.stride(0) >= features.shape[1]):
        return False
    n = rois.shape[0]
    return 1 <= k <= MAX_K and k <= n <= N.kmeans_capacity() and features.shape[0] == n and threshold >= 1 and rois.shape[1] >= 5


def _host_path(rois, features, k, threshold, why):
    from scda_amd.dropin.functions import mask
    logger.debug("cluster_targets: host path for this call (%s)", why)
    return mask.host_cluster_targets(rois, features, k, threshold)


def _pinned(dev):
    """the device's two pinned staging buffers, kept for the life of the process: `host` receives counts, centres and status, `rois`
    sends the RoI rows.  Both transfers run on the side stream and are complete when cluster_targets has synchronised it, so the
    next call may overwrite them."""
    p = _PINNED.get(dev.index)
    if p is None:
        p = _PINNED[dev.index] = {"host": torch.zeros(3 * MAX_K + 2, dtype=torch.int32, pin_memory=True),
                                  "rois": torch.zeros((N.kmeans_capacity(), 5), dtype=torch.float32, pin_memory=True)}
    return p


def cluster_targets(rois, features, N_cluster=4, threshold=128):
    """functions/mask.py:193-237: rois [n, >=5] (b, x1, y1, x2, y2, ...), features [n, F] float32 on the device ->
    (cluster features float32 [N_cluster, threshold, F] on the device (a new leaf), centres float32 numpy [N_cluster, 2])"""
    k, threshold = int(N_cluster), int(threshold)
    if not _covered(rois, features, k, threshold):
        return _host_path(rois, features, k, threshold, "not covered")
    n = rois.shape[0]
    dev = features.device
    main = torch.cuda.current_stream(dev)
    aux = backend._aux_stream(dev)
    first, uniforms, _ = seeding_constants(n, k)
    host_rows = getattr(rois, "_scda_host", None)
    if host_rows is None and not (torch.is_tensor(rois) and rois.is_cuda):
        host_rows = backend.host_array(rois)
    pinned = _pinned(dev)
    host = pinned["host"]
    with torch.cuda.stream(aux):
        if host_rows is not None:     # a pinned upload of the (tiny) rows on the side stream: no dependence on the compute stream at all
            pin = pinned["rois"][:n]
            pin.numpy()[:] = host_rows[:, :5]
            r = pin.to(dev, non_blocking=True)
        else:
            aux.wait_stream(main)
            r = rois.detach().float().contiguous()
        # one buffer for every output: [centres 2k | counts k | n_iter | status | seed_index k | labels n | members k*n]
        work = torch.empty(3 * k + 2 + k + n + k * n, dtype=torch.int32, device=dev)
        head = 3 * k + 2
        bufs = {"centres": work[:2 * k].view(torch.float32), "counts": work[2 * k:3 * k], "n_iter": work[3 * k:3 * k + 1],
                "status": work[3 * k + 1:head], "seed_index": work[head:head + k], "labels": work[head + k:head + k + n],
                "members": work[head + k + n:]}
        N.kmeans(r, k, first, uniforms, bufs)
        host[:head].copy_(work[:head], non_blocking=True)
        aux.synchronize()
    hv = host.numpy()
    if int(hv[3 * k + 1]) != 0:       # a cluster went empty (sklearn's relocation is not restated) or a point is not finite (sklearn raises);
        # the global generator is untouched so far
        return _host_path(rois, features, k, threshold, "kernel status %d" % int(hv[3 * k + 1]))
    counts = hv[2 * k:3 * k].copy()
    centres = hv[:2 * k].view(np.float32).reshape(k, 2).copy()
    picks = None
    if (counts < threshold).any():
        # a fresh pinned block (from torch's pinned cache) per call: this copy runs on the COMPUTE stream, behind its backlog, so a
        # kept buffer could only be reused after waiting for that backlog
        p = torch.zeros((k, threshold), dtype=torch.int32, pin_memory=True)
        pv = p.numpy()
        for c in range(k):            # the reference's draws, in its order (:215-220)
            if counts[c] < threshold:
                pv[c] = np.random.choice(int(counts[c]), threshold, replace=True)
        picks = p.to(dev, non_blocking=True)
    work.record_stream(main)
    with torch.no_grad():
        out = N.cluster_gather(features.detach(), bufs["members"], bufs["counts"], picks, k, threshold)
    return out, centres
