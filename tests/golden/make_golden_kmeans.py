#!/usr/bin/env python
"""Generate tests/golden/kmeans_ref.npz (data only) for the cluster-region generator on the device.

Run in the build container only:   python tests/golden/make_golden_kmeans.py

Every set is a list of RoI rows (b, x1, y1, x2, y2) float32 in a 1024 x 512 image.  What is recorded per set:
  * rows / centres: the REFERENCE's own functions/mask.py:compute_cluster_targets (imported unmodified through ref_harness.py) on
    index-coded features (features[i, :] = i, so the returned tensor spells out the selected RoI rows, the seeded global-RNG draws
    included), np.random.seed(rng_seed) before the call, and the global generator's state after it (rng_keys / rng_pos);
  * labels, seed indices, n_iter: sklearn.cluster.KMeans(k, random_state=0) on the same float32 points (the installed sklearn; its
    version is recorded -- the rule restates 1.7.2), seed indices by replaying its own _kmeans_plusplus;
  * corners: the reference's own get_corner_from_center (tools/faster_rcnn_train_val.py:411-438) on the centres.

Classes (N, k, threshold): the workload's (512, 4, 128) as uniform / object-clustered / padded-by-resampling RoI lists, the reference
driver's other valid pairs (512, 2, 256) and (512, 8, 64), N = 300, N = 96 (every cluster smaller than threshold), N = 16; sets found
by seeded search in which one cluster has exactly threshold, threshold - 1 and threshold + 1 members; and the fallback class (fewer
than k distinct points: sklearn relocates empty clusters, which the rule does not restate).

Selection condition: a set enters the equality fixtures (`equal` = 1) only if tests/kmeans_np.py agrees with sklearn on seeds, labels
and crop corners.  `tried` and `kept` are stored per set class; tests/test_kmeans_rules.py asserts kept >= 95 % of tried overall and
that no (k, N) class is empty.  Sets that were tried and not kept stay in the file with `equal` = 0."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import kmeans_np as KN  # noqa: E402
from make_golden import CFG_PATH  # noqa: E402

W, H = 1024, 512


def _boxes(cx, cy, w, h):
    x1, y1 = np.clip(cx - w / 2, 0, W - 1), np.clip(cy - h / 2, 0, H - 1)
    x2, y2 = np.clip(cx + w / 2, 0, W - 1), np.clip(cy + h / 2, 0, H - 1)
    return np.stack([np.zeros_like(x1), x1, y1, x2, y2], axis=1).astype(np.float32)


def rois_uniform(r, n):
    return _boxes(r.uniform(0, W, n), r.uniform(0, H, n), np.exp(r.uniform(np.log(8), np.log(400), n)), np.exp(r.uniform(np.log(8), np.log(300), n)))


def rois_objects(r, n):
    """RoIs scattered around 2-8 objects, as the proposals of a trained RPN are"""
    g = r.randint(2, 9)
    ox, oy = r.uniform(60, W - 60, g), r.uniform(40, H - 40, g)
    ow, oh = np.exp(r.uniform(np.log(24), np.log(300), g)), np.exp(r.uniform(np.log(24), np.log(200), g))
    of = r.randint(0, g, n)
    return _boxes(ox[of] + r.normal(0, 0.25, n) * ow[of], oy[of] + r.normal(0, 0.25, n) * oh[of],
                  ow[of] * np.exp(r.normal(0, 0.3, n)), oh[of] * np.exp(r.normal(0, 0.3, n)))


def rois_padded(r, n):
    """fewer distinct RoIs than n, padded by resampling with replacement (functions/proposal_target.py:149-155): duplicate rows"""
    m = r.randint(max(n // 8, 8), max(n // 2, 9))
    base = rois_objects(r, m) if r.randint(2) else rois_uniform(r, m)
    return np.concatenate([base, base[r.choice(m, n - m, replace=True)]], axis=0)


KINDS = {"uniform": rois_uniform, "objects": rois_objects, "padded": rois_padded}


def sklearn_run(rois, k):
    """labels, n_iter, centres and the k-means++ seed indices of KMeans(k, random_state=0) on the float32 RoI centres"""
    from sklearn.cluster import KMeans
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms
    X = KN.roi_centres(rois)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, random_state=0).fit(X)
    Xc = X - X.mean(axis=0)
    _, seeds = _kmeans_plusplus(Xc, k, x_squared_norms=row_norms(Xc, squared=True), sample_weight=np.ones(X.shape[0], dtype=X.dtype),
                                random_state=np.random.RandomState(0))
    return km.labels_.astype(np.int32), int(km.n_iter_), km.cluster_centers_, seeds.astype(np.int32)


def reference_call(ns, rois, k, threshold, rng_seed):
    """-> (rows int32 [k, threshold], centres, rng keys, rng pos) of the reference's compute_cluster_targets, or None where it raises"""
    feats = torch.arange(rois.shape[0], dtype=torch.float32)[:, None].repeat(1, 4)
    np.random.seed(rng_seed)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cf, centres = ns.mask.compute_cluster_targets(torch.from_numpy(rois), feats, N_cluster=k, threshold=threshold)
    except ValueError:
        return None
    st = np.random.get_state()
    return cf.numpy()[:, :, 0].astype(np.int32), np.asarray(centres), st[1].copy(), int(st[2])


def main():
    ns = rh.import_reference_driver(["--config", CFG_PATH, "--port", "1", "--dataset", "cityscapes", "--datadir", "x",
                                     "--arch", "vgg16_FasterRCNN", "--dist", "0", "--cluster_num", "4",
                                     "--threshold", "128", "--recon_size", "256"])
    corners_of = lambda c: np.array(ns.T.get_corner_from_center(c), dtype=np.int32)  # noqa: E731
    plan = [(512, 4, 128, 4), (512, 2, 256, 2), (512, 8, 64, 2), (300, 4, 128, 2), (96, 4, 128, 1), (16, 4, 128, 1)]
    sets = []                                     # (name, N, k, threshold, kind, rois)
    seed = 0
    for N, k, thr, per_kind in plan:
        for kind in KINDS:
            for _ in range(per_kind):
                seed += 1
                sets.append(("%s_%d_%d_%d" % (kind, N, k, seed), N, k, thr, kind, KINDS[kind](np.random.RandomState(seed), N)))
    # one cluster with exactly threshold / threshold - 1 / threshold + 1 members: the first seeds at which sklearn's labels say so
    for delta in (0, -1, 1):
        for s in range(5000, 9000):
            rois = rois_uniform(np.random.RandomState(s), 512)
            if (np.bincount(sklearn_run(rois, 4)[0], minlength=4) == 128 + delta).any():
                sets.append(("count_thr%+d_%d" % (delta, s), 512, 4, 128, "boundary", rois))
                break
        else:
            raise RuntimeError("no set with a cluster of %d members found" % (128 + delta))
    d = {"sklearn_version": np.array(__import__("sklearn").__version__), "image_wh": np.array([W, H], dtype=np.int32), "recon": np.array(256)}
    names, tried, kept = [], {}, {}
    for i, (name, N, k, thr, kind, rois) in enumerate(sets):
        labels, n_iter, sk_centres, seeds = sklearn_run(rois, k)
        ref = reference_call(ns, rois, k, thr, 1000 + i)
        assert ref is not None, name
        rows, centres, keys, pos = ref
        corners = corners_of(centres)
        km = KN.kmeans(rois, k)
        equal = int(km["status"] == 0 and np.array_equal(km["seed_index"], seeds) and np.array_equal(km["labels"], labels)
                    and np.array_equal(corners_of(km["centres"]), corners))
        cls = "%d_%d" % (k, N)
        tried[cls] = tried.get(cls, 0) + 1
        kept[cls] = kept.get(cls, 0) + equal
        names.append(name)
        p = "s%02d_" % i
        d.update({p + "rois": rois, p + "k": np.array(k), p + "threshold": np.array(thr), p + "rng_seed": np.array(1000 + i),
                  p + "labels": labels.astype(np.int16), p + "seed_index": seeds, p + "n_iter": np.array(n_iter),
                  p + "rows": rows.astype(np.int16), p + "centres": np.asarray(centres, dtype=np.float32), p + "corners": corners,
                  p + "rng_keys": keys, p + "rng_pos": np.array(pos), p + "equal": np.array(equal)})
        print("%-28s N %4d k %d n_iter %3d counts %s equal %d |centres - numpy| %.2e" % (
            name, N, k, n_iter, np.bincount(labels, minlength=k).tolist(), equal,
            np.abs(km["centres"] - centres).max() if km["status"] == 0 else float("nan")))
    d["names"] = np.array(names)
    d["classes"] = np.array(sorted(tried))
    d["tried"] = np.array([tried[c] for c in sorted(tried)], dtype=np.int32)
    d["kept"] = np.array([kept[c] for c in sorted(tried)], dtype=np.int32)
    # the fallback class: fewer than k distinct points -> an empty cluster during Lloyd (sklearn relocates it; the rule raises its flag)
    fb = []
    for j, (N, k, thr, distinct) in enumerate([(64, 4, 128, 3), (512, 4, 128, 2), (16, 8, 64, 5)]):
        r = np.random.RandomState(700 + j)
        base = rois_uniform(r, distinct)
        rois = base[np.concatenate([np.arange(distinct), r.randint(0, distinct, N - distinct)])]
        ref = reference_call(ns, rois, k, thr, 2000 + j)
        p = "f%02d_" % j
        d.update({p + "rois": rois, p + "k": np.array(k), p + "threshold": np.array(thr), p + "rng_seed": np.array(2000 + j),
                  p + "raises": np.array(int(ref is None))})
        if ref is not None:
            d.update({p + "rows": ref[0].astype(np.int16), p + "centres": np.asarray(ref[1], dtype=np.float32), p + "rng_keys": ref[2],
                      p + "rng_pos": np.array(ref[3])})
        fb.append("fewer_distinct_%d_%d_%d" % (N, k, distinct))
        print("%-28s reference raises: %s; numpy status %d" % (fb[-1], ref is None, KN.kmeans(rois, k)["status"]))
    d["fallback_names"] = np.array(fb)
    out = os.path.join(HERE, "kmeans_ref.npz")
    np.savez_compressed(out, **d)
    print("kmeans_ref.npz written: %d sets, kept %d of %d; %d fallback sets; %d bytes" % (
        len(sets), int(d["kept"].sum()), int(d["tried"].sum()), len(fb), os.path.getsize(out)))


if __name__ == "__main__":
    main()
