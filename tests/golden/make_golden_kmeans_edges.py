#!/usr/bin/env python
"""Generate tests/golden/kmeans_edges_ref.npz (data only): scikit-learn's own answer on the cases of tests/kmeans_edge_cases.py.

Run where scikit-learn 1.7.2 is installed (the version the rule of include/scda_ops.h restates):
    python tests/golden/make_golden_kmeans_edges.py

Per case: the RoI rows (each distinct array once, `roi_index` says which), k, threshold, and what make_golden_kmeans.py:sklearn_run
records -- the labels (int16), n_iter and centres of sklearn.cluster.KMeans(k, random_state=0) on the float32 RoI centres and the
k-means++ seed indices from a replay of its _kmeans_plusplus.  sklearn runs on ONE OpenMP thread here: its Lloyd step sums the
centres per thread and joins the threads in the order they finish, so only then do two runs of it give the same float32 centres.
The reference's compute_cluster_targets is not called: tests/golden/kmeans_ref.npz pins that already.

Selection condition, that of kmeans_ref.npz: `equal` = 1 where tests/kmeans_np.py ends with status 0 and agrees with sklearn on seeds,
labels and crop corners (scda_amd.train_step.get_corner_from_center, 256 px windows), and here also on n_iter and on the centres
within 1e-3 px, which tests/test_kmeans_edges_rules.py then asserts.  `differs` names the first field that disagrees.  `tried` and
`kept` are stored per class; the test asserts kept >= 95 % of tried and kept > 0 in every class.  A case that is not kept stays in
the file with `equal` = 0: the kernel must equal the numpy statement on it all the same.  The fallback class (fewer than k distinct
points) is stored as rows only and is no part of `tried`."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import kmeans_np as KN  # noqa: E402
import kmeans_edge_cases as EC  # noqa: E402

CENTRE_ATOL = 1e-3
RECON = 256


def sklearn_run(rois, k):
    """labels, n_iter, centres and the k-means++ seed indices of KMeans(k, random_state=0) on the float32 RoI centres"""
    from sklearn.cluster import KMeans
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms
    from threadpoolctl import threadpool_limits
    X = KN.roi_centres(rois)
    with warnings.catch_warnings(), threadpool_limits(limits=1):
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, random_state=0).fit(X)
        Xc = X - X.mean(axis=0)
        _, seeds = _kmeans_plusplus(Xc, k, x_squared_norms=row_norms(Xc, squared=True), sample_weight=np.ones(X.shape[0], dtype=X.dtype),
                                    random_state=np.random.RandomState(0))
    return km.labels_.astype(np.int32), int(km.n_iter_), np.asarray(km.cluster_centers_, dtype=np.float32), seeds.astype(np.int32)


def corners_of(centres):
    from scda_amd.train_step import get_corner_from_center
    return np.array(get_corner_from_center(centres, RECON, EC.W, EC.H), dtype=np.int32)


def first_difference(km, labels, n_iter, centres, seeds):
    """'' where the numpy statement agrees with sklearn, else the first field in which it does not"""
    if km["status"] != 0:
        return "status"
    if not np.array_equal(km["seed_index"], seeds):
        return "seed_index"
    if not np.array_equal(km["labels"], labels):
        return "labels"
    if km["n_iter"] != n_iter:
        return "n_iter"
    if not np.allclose(km["centres"], centres, rtol=0, atol=CENTRE_ATOL):
        return "centres"
    if not np.array_equal(corners_of(km["centres"]), corners_of(centres)):
        return "corners"
    return ""


def main():
    import sklearn
    d = {"sklearn_version": np.array(sklearn.__version__), "image_wh": np.array([EC.W, EC.H], dtype=np.int32), "recon": np.array(RECON)}
    cases = EC.cases()
    unique = []                                    # each distinct RoI array once
    names, classes, differs, ks, thrs, roi_index, n_iters, equals = [], [], [], [], [], [], [], []
    tried, kept = {}, {}
    for i, (name, cls, rois, k, thr) in enumerate(cases):
        for j, u in enumerate(unique):
            if u is rois:
                break
        else:
            j = len(unique)
            unique.append(rois)
            d["rois_%03d" % j] = rois
        labels, n_iter, centres, seeds = sklearn_run(rois, k)
        diff = first_difference(KN.kmeans(rois, k), labels, n_iter, centres, seeds)
        tried[cls] = tried.get(cls, 0) + 1
        kept[cls] = kept.get(cls, 0) + (diff == "")
        names.append(name); classes.append(cls); differs.append(diff); ks.append(k); thrs.append(thr); roi_index.append(j)
        n_iters.append(n_iter); equals.append(int(diff == ""))
        d.update({"labels_%03d" % i: labels.astype(np.int16), "centres_%03d" % i: centres, "seeds_%03d" % i: seeds})
        print("%-22s %-10s N %4d k %d n_iter %3d counts %-40s %s" % (name, cls, rois.shape[0], k, n_iter, np.bincount(labels, minlength=k).tolist(),
                                                                    "equal" if not diff else "DIFFERS in " + diff))
    d.update(names=np.array(names), case_class=np.array(classes), differs=np.array(differs), k=np.array(ks, dtype=np.int32),
             threshold=np.array(thrs, dtype=np.int32), roi_index=np.array(roi_index, dtype=np.int32), n_iter=np.array(n_iters, dtype=np.int32),
             equal=np.array(equals, dtype=np.int32), classes=np.array(sorted(tried)),
             tried=np.array([tried[c] for c in sorted(tried)], dtype=np.int32), kept=np.array([kept[c] for c in sorted(tried)], dtype=np.int32))
    fb = EC.fallback_cases()
    for j, (name, _, rois, k, thr) in enumerate(fb):
        d["fb_rois_%d" % j] = rois
        print("%-22s fallback   N %4d k %d numpy status %d" % (name, rois.shape[0], k, KN.kmeans(rois, k)["status"]))
    d.update(fb_names=np.array([c[0] for c in fb]), fb_k=np.array([c[3] for c in fb], dtype=np.int32),
             fb_threshold=np.array([c[4] for c in fb], dtype=np.int32))
    out = os.path.join(HERE, "kmeans_edges_ref.npz")
    np.savez_compressed(out, **d)
    print("\nclass       tried kept")
    for c in sorted(tried):
        print("%-11s %5d %4d" % (c, tried[c], kept[c]))
    print("%-11s %5d %4d  (%.1f %%)" % ("all", sum(tried.values()), sum(kept.values()), 100.0 * sum(kept.values()) / sum(tried.values())))
    print("kmeans_edges_ref.npz written: %d cases, %d RoI arrays, %d fallback cases, %d bytes" % (len(cases), len(unique), len(fb), os.path.getsize(out)))


if __name__ == "__main__":
    main()
