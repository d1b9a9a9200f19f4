"""COCO detection evaluation in plain numpy: a restatement of the rules include/scda_ops.h states for scda_amd/csrc/coco_eval.hip
(bbIou, COCOeval.evaluateImg / accumulate / _summarizeDets for iouType 'bbox' / 'segm' with useCats = 1).  It is the second statement
of those rules: tests/test_coco_eval_rules.py holds it against the arrays recorded from the reference's own code
(tests/golden/coco_eval_ref.npz), the GPU tests and scripts/time_coco_eval.py hold the kernels against it.

An image is a dict of arrays: image_id, dt_xywh f64 [D, 4], dt_score f32 [D], dt_cat i32 [D] (1..K), dt_area f64 [D], gt_xywh f64 [G, 4],
gt_area f64 [G], gt_iscrowd u8 [G], gt_cat i32 [G], iou f64 [G, D] (o[g, d], every pair of the image)."""
import numpy as np

EPS = 2.220446049250313e-16                     # np.spacing(1)


def default_params():
    """Params.setDetParams (cocoeval.py:503-512)"""
    return {'iou_thrs': np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            'rec_thrs': np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            'max_dets': [1, 10, 100],
            'area_rng': np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)}


def xywh_from_corners(corners):
    """float32 [n, 4] (x1, y1, x2, y2) -> float64 (x, y, w, h), w = (double) x2 - (double) x1"""
    c = np.asarray(corners, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    return np.stack([c[:, 0], c[:, 1], c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]], 1)


def bb_iou(dt, gt, iscrowd):
    """maskApi.c:110-121 -> o [G, D]"""
    o = np.zeros((len(gt), len(dt)), dtype=np.float64)
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if iscrowd[g] else da + ga - i
            o[g, d] = i / u
    return o


def evaluate_image(img, K, iou_thrs, area_rng, max_det):
    """evaluateImg for every category, area range and threshold of one image ->
    rank i32 [D] (within (image, category); every detection has one), match i32 [D, A, T] (the matched GT's row or -1), ignore bool
    [D, A, T], gt_ignore bool [G, A], npig i32 [K, A], seen bool [K].  Detections of rank >= max_det take no part (-1 / False)."""
    T, A = len(iou_thrs), len(area_rng)
    D, G = len(img['dt_score']), len(img['gt_cat'])
    rank = np.full(D, -1, dtype=np.int32)
    match = np.full((D, A, T), -1, dtype=np.int32)
    ignore = np.zeros((D, A, T), dtype=bool)
    gt_ignore = np.zeros((G, A), dtype=bool)
    npig = np.zeros((K, A), dtype=np.int32)
    seen = np.zeros(K, dtype=bool)
    for k in range(1, K + 1):
        dl = np.flatnonzero(img['dt_cat'] == k)
        gl = np.flatnonzero(img['gt_cat'] == k)
        if len(dl) == 0 and len(gl) == 0:
            continue
        seen[k - 1] = True
        order = np.argsort(-img['dt_score'][dl].astype(np.float64), kind='mergesort')
        rank[dl[order]] = np.arange(len(dl))
        dts = dl[order][:max_det]
        for a, (lo, hi) in enumerate(area_rng):
            ig = np.array([bool(img['gt_iscrowd'][g]) or img['gt_area'][g] < lo or img['gt_area'][g] > hi for g in gl], dtype=bool)
            gt_ignore[gl, a] = ig
            gts = gl[np.argsort(ig, kind='mergesort')]
            gig = np.sort(ig, kind='mergesort')
            npig[k - 1, a] = int((~ig).sum())
            crowd = [bool(img['gt_iscrowd'][g]) for g in gts]
            for t, thr in enumerate(iou_thrs):
                gtm = np.zeros(len(gts), dtype=bool)
                for d in dts:
                    best, m = min(thr, 1 - 1e-10), -1
                    for gi, g in enumerate(gts):
                        if gtm[gi] and not crowd[gi]:
                            continue
                        if m > -1 and not gig[m] and gig[gi]:
                            break
                        if img['iou'][g, d] < best:
                            continue
                        best, m = img['iou'][g, d], gi
                    if m == -1:
                        ignore[d, a, t] = img['dt_area'][d] < lo or img['dt_area'][d] > hi
                        continue
                    gtm[m] = True
                    match[d, a, t] = gts[m]
                    ignore[d, a, t] = gig[m]
    return {'rank': rank, 'match': match, 'ignore': ignore, 'gt_ignore': gt_ignore, 'npig': npig, 'seen': seen}


def accumulate(images, per_image, K, iou_thrs, rec_thrs, area_rng, max_dets):
    """accumulate (cocoeval.py:316-419) over the images in ascending image id -> precision [T, R, K, A, M], recall [T, K, A, M],
    scores [T, R, K, A, M]"""
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_rng), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    by_id = np.argsort([int(im['image_id']) for im in images], kind='mergesort')
    seen = np.zeros(K, dtype=bool)
    npig = np.zeros((K, A), dtype=np.int64)
    for e in per_image:
        seen |= e['seen']
        npig += e['npig']
    for k in range(K):
        if not seen[k]:
            continue
        # the category's rows, image by image, in rank order
        sc, rk, mt, ig = [], [], [], []
        for i in by_id:
            im, e = images[i], per_image[i]
            dl = np.flatnonzero((im['dt_cat'] == k + 1) & (e['rank'] < max_dets[-1]))
            dl = dl[np.argsort(e['rank'][dl], kind='mergesort')]
            sc.append(im['dt_score'][dl].astype(np.float64)); rk.append(e['rank'][dl])
            mt.append(e['match'][dl] >= 0); ig.append(e['ignore'][dl])
        sc, rk = np.concatenate(sc), np.concatenate(rk)
        mt, ig = np.concatenate(mt), np.concatenate(ig)                       # [n, A, T]
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for m, max_det in enumerate(max_dets):
                sub = np.flatnonzero(rk < max_det)
                inds = sub[np.argsort(-sc[sub], kind='mergesort')]
                ss = sc[inds]
                nd = len(inds)
                for t in range(T):
                    dtm, dti = mt[inds, a, t], ig[inds, a, t]
                    tp = np.cumsum(dtm & ~dti).astype(np.float64)
                    fp = np.cumsum(~dtm & ~dti).astype(np.float64)
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + EPS)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q, s = np.zeros(R), np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side='left')):
                        if pi >= nd:
                            break
                        q[ri], s[ri] = pr[pi], ss[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = s
    return precision, recall, scores


def stat_specs(iou_thrs, max_dets):
    """_summarizeDets' 12 selections as (ap, t, a, m): t = -1 every threshold, -2 a threshold the list does not hold (the reference's
    np.where(iouThr == p.iouThrs) then selects nothing); area ranges in the order all, small, medium, large.  The maxDets entry is the
    reference's (cocoeval.py:459-472): maxDets[2] for stats 1..5 and 8..11, maxDets[0] / maxDets[1] for stats 6 / 7, and for stat 0
    (_summarize(1), default maxDets = 100) the entry EQUAL to 100 -- nothing, hence -1, when the list holds no 100.  Fewer than three
    entries, where the reference raises IndexError: the missing entries fall back to the last one"""
    def at(v):
        w = np.where(v == np.asarray(iou_thrs))[0]
        return int(w[0]) if len(w) else -2
    max_dets = [int(m) for m in max_dets]
    last = len(max_dets) - 1
    m1, m2 = min(1, last), min(2, last)
    t100, m100 = (-1, max_dets.index(100)) if 100 in max_dets else (-2, 0)
    return np.array([(1, t100, 0, m100), (1, at(.5), 0, m2), (1, at(.75), 0, m2), (1, -1, 1, m2), (1, -1, 2, m2), (1, -1, 3, m2),
                     (0, -1, 0, 0), (0, -1, 0, m1), (0, -1, 0, m2), (0, -1, 1, m2), (0, -1, 2, m2), (0, -1, 3, m2)],
                    dtype=np.int32)


def summarize(precision, recall, specs):
    stats = np.zeros(len(specs))
    for i, (ap, t, a, m) in enumerate(specs):
        s = precision if ap else recall
        s = s[:0] if t == -2 else (s if t == -1 else s[t:t + 1])
        s = s[..., a, m]
        stats[i] = np.mean(s[s > -1]) if len(s[s > -1]) else -1
    return stats


def stat_counts(precision, recall, specs):
    """the number of averaged entries of each stat (the N of the 2 N 2^-53 bound between two summation orders)"""
    n = []
    for ap, t, a, m in specs:
        s = precision if ap else recall
        s = s[:0] if t == -2 else (s if t == -1 else s[t:t + 1])
        n.append(int((s[..., a, m] > -1).sum()))
    return np.asarray(n)


def evaluate(images, K, params=None):
    """-> dict: per_image (evaluate_image's results), precision, recall, scores, stats"""
    p = dict(default_params(), **(params or {}))
    per = [evaluate_image(im, K, p['iou_thrs'], p['area_rng'], p['max_dets'][-1]) for im in images]
    precision, recall, scores = accumulate(images, per, K, p['iou_thrs'], p['rec_thrs'], p['area_rng'], p['max_dets'])
    specs = stat_specs(p['iou_thrs'], p['max_dets'])
    return {'per_image': per, 'precision': precision, 'recall': recall, 'scores': scores,
            'stats': summarize(precision, recall, specs), 'specs': specs}


def load_set(z, name):
    """one set of tests/golden/coco_eval_ref.npz -> (images, K, params): the flat arrays cut into per-image dicts"""
    dc, gc = z[name + '_dt_counts'], z[name + '_gt_counts']
    do, go = np.concatenate([[0], np.cumsum(dc)]), np.concatenate([[0], np.cumsum(gc)])
    io = np.concatenate([[0], np.cumsum(dc.astype(np.int64) * gc)])
    xywh = xywh_from_corners(z[name + '_dt_corners'])
    images = []
    for i in range(len(dc)):
        d, g = slice(do[i], do[i + 1]), slice(go[i], go[i + 1])
        images.append({'image_id': int(z[name + '_image_ids'][i]), 'dt_corners': z[name + '_dt_corners'][d], 'dt_xywh': xywh[d],
                       'dt_score': z[name + '_dt_scores'][d], 'dt_cat': z[name + '_dt_cats'][d], 'dt_area': z[name + '_dt_areas'][d],
                       'gt_xywh': z[name + '_gt_boxes'][g], 'gt_area': z[name + '_gt_areas'][g], 'gt_iscrowd': z[name + '_gt_iscrowd'][g],
                       'gt_cat': z[name + '_gt_cats'][g], 'iou': z[name + '_iou'][io[i]:io[i + 1]].reshape(int(gc[i]), int(dc[i])),
                       'dt': d, 'gt': g})
    params = default_params()
    params['area_rng'] = z[name + '_area_rng']
    return images, int(z[name + '_K']), params
