"""COCO keypoint (OKS) and category-agnostic (useCats = 0) evaluation in plain numpy: a restatement of the rules include/scda_ops.h
states for scda_coco_kp_rows_hip, scda_coco_oks_hip, scda_coco_match_ign_hip, scda_coco_regroup_hip, scda_coco_prop_rows_hip and the
ten specs of _summarizeKps.  Everything else -- accumulate, summarize, the 12 specs -- is tests/coco_eval_np.py's.
tests/test_coco_kps_rules.py holds it against the arrays recorded from the reference's own code (tests/golden/coco_kps_ref.npz), the
GPU tests hold the kernels against it.

An image is coco_eval_np's dict; a keypoint image also has dt_kps f32 [D, Kp, 3], gt_kps f64 [G, Kp, 3], gt_num_kps i32 [G], and
gt_ignore u8 [G] (the GT's own ignore flag; without the key it is gt_iscrowd)."""
import numpy as np

import coco_eval_np as cnp

EPS = cnp.EPS


def default_params():
    """Params.setKpParams (cocoeval.py:514-523) and computeOks' sigmas (:206)"""
    p = cnp.default_params()
    p['max_dets'] = [20]
    p['area_rng'] = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
    p['sigmas'] = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
    return p


def kp_rows(dt_kps):
    """loadRes for keypoint results (coco.py:350-357): float32 [D, Kp, 3] -> xywh f64 [D, 4], area f64 [D]: the extent of ALL Kp points"""
    if len(dt_kps) == 0:
        return np.zeros((0, 4)), np.zeros(0)
    k = np.asarray(dt_kps, dtype=np.float32).astype(np.float64).reshape(len(dt_kps), -1, 3)
    x0, x1, y0, y1 = k[:, :, 0].min(1), k[:, :, 0].max(1), k[:, :, 1].min(1), k[:, :, 1].max(1)
    return np.stack([x0, y0, x1 - x0, y1 - y0], 1), (x1 - x0) * (y1 - y0)


def oks_terms(d, g, bb, area, var):
    """one pair: (e of the counted keypoints, in keypoint order).  d f64 [Kp, 3], g f64 [Kp, 3]"""
    vis = g[:, 2] > 0
    if vis.any():
        dx, dy = d[:, 0] - g[:, 0], d[:, 1] - g[:, 1]
    else:
        x0, x1 = bb[0] - bb[2], bb[0] + bb[2] * 2
        y0, y1 = bb[1] - bb[3], bb[1] + bb[3] * 2
        dx = np.maximum(0.0, x0 - d[:, 0]) + np.maximum(0.0, d[:, 0] - x1)
        dy = np.maximum(0.0, y0 - d[:, 1]) + np.maximum(0.0, d[:, 1] - y1)
    e = (dx * dx + dy * dy) / var / (area + EPS) / 2
    return e[vis] if vis.any() else e


def oks(dt_kps, gt_kps, gt_xywh, gt_area, sigmas):
    """computeOks (cocoeval.py:193-234) for every pair of an image -> o [G, D]; the sum runs in ascending keypoint order"""
    var = (np.asarray(sigmas, dtype=np.float64) * 2) ** 2
    d64 = np.asarray(dt_kps, dtype=np.float32).astype(np.float64)
    o = np.zeros((len(gt_kps), len(d64)), dtype=np.float64)
    for g in range(len(gt_kps)):
        for d in range(len(d64)):
            e = oks_terms(d64[d], np.asarray(gt_kps[g], dtype=np.float64), gt_xywh[g], gt_area[g], var)
            s = 0.0
            for v in np.exp(-e):
                s = s + v
            o[g, d] = s / len(e)
    return o


def kp_gt_ignore(gt_iscrowd, gt_num_kps):
    """gt['ignore'] = iscrowd || num_keypoints == 0 (cocoeval.py:108-112)"""
    return ((np.asarray(gt_iscrowd) != 0) | (np.asarray(gt_num_kps) == 0)).astype(np.uint8)


def evaluate_image(img, K, iou_thrs, area_rng, max_det):
    """coco_eval_np.evaluate_image with the GT's ignore flag (img['gt_ignore'], default gt_iscrowd) apart from its iscrowd, which alone
    decides whether a matched GT may be matched again"""
    T, A = len(iou_thrs), len(area_rng)
    D, G = len(img['dt_score']), len(img['gt_cat'])
    gign = np.asarray(img.get('gt_ignore', img['gt_iscrowd']))
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
            ig = np.array([bool(gign[g]) or img['gt_area'][g] < lo or img['gt_area'][g] > hi for g in gl], dtype=bool)
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


def regroup_order(cats, K):
    """useCats = 0: the indices with 1 <= cat <= K in (category ascending, given order) order -- the concatenation of the categories'
    lists (cocoeval.py:169-171, 245-247)"""
    cats = np.asarray(cats)
    live = np.flatnonzero((cats >= 1) & (cats <= K))
    return live[np.argsort(cats[live], kind='mergesort')]


def regroup(img, K):
    """-> (the image with its rows in the useCats = 0 order and every category 1, perm_dets, perm_gts)"""
    pd, pg = regroup_order(img['dt_cat'], K), regroup_order(img['gt_cat'], K)
    out = {'image_id': img['image_id'], 'dt_xywh': img['dt_xywh'][pd], 'dt_score': img['dt_score'][pd], 'dt_area': img['dt_area'][pd],
           'dt_cat': np.ones(len(pd), np.int32), 'gt_xywh': img['gt_xywh'][pg], 'gt_area': img['gt_area'][pg],
           'gt_iscrowd': img['gt_iscrowd'][pg], 'gt_cat': np.ones(len(pg), np.int32),
           'iou': np.asarray(img['iou']).reshape(len(img['gt_cat']), len(img['dt_score']))[pg][:, pd]}
    return out, pd, pg


def proposal_xywh(corners, xyxy_as_xywh=False):
    """float32 [n, 4] (x1, y1, x2, y2) -> float64 (x, y, w, h); xyxy_as_xywh: (x2, y2) taken as (w, h), utils/coco_eval.py:33-36"""
    c = np.asarray(corners, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    return c.copy() if xyxy_as_xywh else cnp.xywh_from_corners(corners)


def kps_stat_specs(iou_thrs, max_dets):
    """_summarizeKps' 10 selections (cocoeval.py:474-486) as (ap, t, a, m), t as in coco_eval_np.stat_specs; area ranges in the order
    all, medium, large; the maxDets entry EQUAL to 20, nothing (t = -2) when the list holds no 20"""
    def at(v):
        w = np.where(v == np.asarray(iou_thrs))[0]
        return int(w[0]) if len(w) else -2
    max_dets = [int(m) for m in max_dets]
    have = 20 in max_dets
    m = max_dets.index(20) if have else 0
    rows = []
    for ap in (1, 0):
        for t, a in ((-1, 0), (at(.5), 0), (at(.75), 0), (-1, 1), (-1, 2)):
            rows.append((ap, t if have else -2, a, m))
    return np.array(rows, dtype=np.int32)


def evaluate(images, K, params, keypoints=False, use_cats=True):
    """-> dict: per_image, precision, recall, scores, stats, specs and, with use_cats=False, perm_dets / perm_gts per image (the
    per-image arrays are then in the REGROUPED order, match naming regrouped GT rows)"""
    perms = None
    if not use_cats:
        trip = [regroup(im, K) for im in images]
        images, perms, K = [t[0] for t in trip], [(t[1], t[2]) for t in trip], 1
    per = [evaluate_image(im, K, params['iou_thrs'], params['area_rng'], params['max_dets'][-1]) for im in images]
    precision, recall, scores = cnp.accumulate(images, per, K, params['iou_thrs'], params['rec_thrs'], params['area_rng'], params['max_dets'])
    specs = (kps_stat_specs if keypoints else cnp.stat_specs)(params['iou_thrs'], params['max_dets'])
    return {'per_image': per, 'precision': precision, 'recall': recall, 'scores': scores,
            'stats': cnp.summarize(precision, recall, specs), 'specs': specs, 'perms': perms}


def cut(z, name):
    """the per-image slices of a set of tests/golden/coco_kps_ref.npz -> (dt slices, gt slices, pair offsets)"""
    dc, gc = z[name + '_dt_counts'], z[name + '_gt_counts']
    do, go = np.concatenate([[0], np.cumsum(dc)]), np.concatenate([[0], np.cumsum(gc)])
    io = np.concatenate([[0], np.cumsum(dc.astype(np.int64) * gc)])
    n = len(dc)
    return [slice(do[i], do[i + 1]) for i in range(n)], [slice(go[i], go[i + 1]) for i in range(n)], io


def load_kp_set(z, name, recorded_oks=False):
    """a keypoint set -> (images, K, params); iou = this file's oks(), or the recorded one"""
    ds, gs, io = cut(z, name)
    params = default_params()
    params['area_rng'] = z[name + '_area_rng']
    images = []
    for i, (d, g) in enumerate(zip(ds, gs)):
        q = z[name + '_dt_kps_q'][d]                                          # int16 quarters of a pixel
        kps = np.concatenate([q.astype(np.float32) / 4, np.ones(q.shape[:2] + (1,), np.float32)], 2)
        xywh, area = kp_rows(kps)
        im = {'image_id': int(z[name + '_image_ids'][i]), 'dt_kps': kps, 'dt_xywh': xywh, 'dt_area': area,
              'dt_score': z[name + '_dt_scores'][d], 'dt_cat': z[name + '_dt_cats'][d], 'gt_kps': z[name + '_gt_kps'][g],
              'gt_num_kps': z[name + '_gt_num_kps'][g], 'gt_xywh': z[name + '_gt_boxes'][g], 'gt_area': z[name + '_gt_areas'][g],
              'gt_iscrowd': z[name + '_gt_iscrowd'][g], 'gt_cat': z[name + '_gt_cats'][g], 'dt': d, 'gt': g}
        im['gt_ignore'] = kp_gt_ignore(im['gt_iscrowd'], im['gt_num_kps'])
        G, D = len(im['gt_cat']), len(im['dt_score'])
        im['oks_ref'] = z[name + '_oks'][io[i]:io[i + 1]].reshape(G, D)
        im['iou'] = im['oks_ref'] if recorded_oks else oks(im['dt_kps'], im['gt_kps'], im['gt_xywh'], im['gt_area'], params['sigmas'])
        images.append(im)
    return images, int(z[name + '_K']), params


def load_box_set(z, name, xyxy_as_xywh=False):
    """a useCats = 0 box set -> (images, K, params)"""
    ds, gs, _ = cut(z, name)
    params = cnp.default_params()
    params['area_rng'] = z[name + '_area_rng']
    params['max_dets'] = [int(m) for m in z[name + '_max_dets']]
    images = []
    for i, (d, g) in enumerate(zip(ds, gs)):
        xywh = proposal_xywh(z[name + '_dt_corners'][d], xyxy_as_xywh)
        im = {'image_id': int(z[name + '_image_ids'][i]), 'dt_corners': z[name + '_dt_corners'][d], 'dt_xywh': xywh,
              'dt_area': xywh[:, 2] * xywh[:, 3], 'dt_score': z[name + '_dt_scores'][d], 'dt_cat': z[name + '_dt_cats'][d],
              'gt_xywh': z[name + '_gt_boxes'][g], 'gt_area': z[name + '_gt_areas'][g], 'gt_iscrowd': z[name + '_gt_iscrowd'][g],
              'gt_cat': z[name + '_gt_cats'][g], 'dt': d, 'gt': g}
        im['iou'] = cnp.bb_iou(xywh, im['gt_xywh'], im['gt_iscrowd'])
        images.append(im)
    return images, int(z[name + '_K']), params
