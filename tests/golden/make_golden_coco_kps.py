"""Generates tests/golden/coco_kps_ref.npz with the REFERENCE's evaluator, as make_golden_coco_eval.py does for coco_eval_ref.npz (its
maskApi.c stand-in and its unmodified import of datasets/pycocotools/coco.py and cocoeval.py are reused): iouType 'keypoints'
(computeOks, setKpParams, _summarizeKps) and useCats = 0 (the reference's 'proposal' test types).  Run in the build container:
    python tests/golden/make_golden_coco_kps.py [path of the reference checkout]
No reference program text is kept; the file holds inputs and recorded outputs only, per set `s`, flat over the images in the order
they are GIVEN, cut by s_dt_counts / s_gt_counts:
  keypoint sets (kp_rules, kp_random, kp_blocks)
    inputs    s_image_ids, s_K, s_area_rng [3, 2], s_dt_kps_q i16 [n, 17, 2] = 4 * (x, y): detections stand on quarter pixels (the third value of a
              detection's keypoint is not read: the loader puts 1 there), s_dt_scores f32, s_dt_cats, s_gt_kps f64 [g, 17, 3],
              s_gt_num_kps (the annotation's field), s_gt_boxes f64 [g, 4] xywh, s_gt_areas, s_gt_iscrowd, s_gt_cats
    recorded  s_oks (per image o[g * D + d] of EVERY pair: computeOks of a second run whose annotations all carry category 1 and whose
              maxDets cuts nothing), and from the run proper s_rank, s_match i32 [n, 3, T], s_ignore u8 [n, 3, T], s_gt_ignore u8
              [g, 3], s_npig [K, 3], s_precision, s_recall, s_scores, s_stats [10] as in coco_eval_ref.npz
  useCats = 0 box sets (nocat_rules: hand-made class rows; nocat_props: seeded proposals and nocat_xyxy: hand-made proposals, every
  category 1, both scored as the reference's 'proposal' run scores them, [x1, y1, x2, y2] handed over as xywh -- in nocat_xyxy that
  reading takes one match away and leaves one)
    inputs    as in coco_eval_ref.npz (s_dt_corners f32 x1, y1, x2, y2 ...) and s_max_dets
    recorded  the same arrays with K = 1; s_match names GT rows of the image in the order GIVEN; s_dt_order / s_gt_order: per image the
              given indices of its detections / GTs in the reference's order (the concatenation over the categories), flat, cut by
              s_dt_live / s_gt_live
  nocat_segm  recorded arrays only: the inputs are random_segm's of coco_eval_ref.npz
s_rank and s_match are stored as int16 (ranks and GT rows stay below 1024), which keeps the file small.
main asserts the coverage of every set and, before it writes, the MARGIN CONDITION that keeps bit-equal comparisons honest although
exp() differs in its last bit between implementations: (1) every recorded OKS is farther than 1e-9 from every IoU threshold; (2) for
every detection any two of its OKS values >= 0.5 - 1e-9 differ by more than 1e-9, unless the two come from bit-identical e vectors.  A
seed that violates it is changed; the margin is not."""
import contextlib
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_coco_eval as base  # noqa: E402
import coco_eval_np as cnp  # noqa: E402
import coco_kps_np as knp  # noqa: E402

KP = 17
MARGIN = 1e-9


# ------------------------------------------------------------------------------------------------------------ the reference runs
def run(coco_mod, eval_mod, images, K, area_rng, iou_type, size=(512, 1024), max_dets=None, use_cats=True, xyxy_as_xywh=False,
        one_category=False):
    """-> (E, first_dt, first_gt): the evaluated COCOeval and the annotation index of every image's first detection / GT"""
    h, w = size
    gt_anns, dt_anns, first_dt, first_gt = [], [], {}, {}
    for im in images:
        first_dt[im['image_id']], first_gt[im['image_id']] = len(dt_anns), len(gt_anns)
        for g in range(len(im['gt_cat'])):
            ann = {'id': len(gt_anns) + 1, 'image_id': im['image_id'], 'category_id': 1 if one_category else int(im['gt_cat'][g]),
                   'bbox': [float(v) for v in im['gt_xywh'][g]], 'area': float(im['gt_area'][g]), 'iscrowd': int(im['gt_iscrowd'][g])}
            if iou_type == 'keypoints':
                ann['keypoints'] = [float(v) for v in im['gt_kps'][g].reshape(-1)]
                ann['num_keypoints'] = int(im['gt_num_kps'][g])
            if iou_type == 'segm':
                ann['segmentation'] = {'size': [h, w], 'counts': b'', 'mask': im['gt_mask'][g]}
            gt_anns.append(ann)
        for d in range(len(im['dt_score'])):
            ann = {'image_id': im['image_id'], 'category_id': 1 if one_category else int(im['dt_cat'][d]), 'score': float(im['dt_score'][d])}
            if iou_type == 'keypoints':
                ann['keypoints'] = [float(v) for v in im['dt_kps'][d].reshape(-1)]        # float32 values as Python floats
            elif iou_type == 'segm':
                ann['segmentation'] = {'size': [h, w], 'counts': b'', 'mask': im['dt_mask'][d]}
            else:
                ann['bbox'] = [float(v) for v in knp.proposal_xywh(im['dt_corners'][d:d + 1], xyxy_as_xywh)[0]]
            dt_anns.append(ann)
    gt = coco_mod.COCO()
    gt.dataset = {'images': [{'id': im['image_id'], 'height': h, 'width': w} for im in images],
                  'categories': [{'id': k} for k in range(1, K + 1)], 'annotations': gt_anns}
    with contextlib.redirect_stdout(io.StringIO()):
        gt.createIndex()
        dt = gt.loadRes(dt_anns)
        E = eval_mod.COCOeval(gt, dt, iou_type)
        E.params.areaRng = [list(map(float, r)) for r in area_rng]
        if max_dets is not None:
            E.params.maxDets = list(max_dets)
        if not use_cats:
            E.params.useCats = 0
        E.evaluate()
        E.accumulate()
        E.summarize()
    return E, first_dt, first_gt


def record(E, images, first_dt, first_gt, K, use_cats=True):
    """evalImgs, eval and stats as flat arrays (see the module's docstring)"""
    A, T = len(E.params.areaRng), len(E.params.iouThrs)
    nd = sum(len(im['dt_score']) for im in images)
    ng = sum(len(im['gt_cat']) for im in images)
    rank = np.full(nd, -1, dtype=np.int32)
    match = np.full((nd, A, T), -1, dtype=np.int32)
    ignore = np.zeros((nd, A, T), dtype=np.uint8)
    gt_ignore = np.zeros((ng, A), dtype=np.uint8)
    KE = K if use_cats else 1
    npig = np.zeros((KE, A), dtype=np.int32)
    ids = sorted(im['image_id'] for im in images)
    I = len(ids)
    for k in range(KE):
        for a in range(A):
            for i in range(I):
                e = E.evalImgs[(k * A + a) * I + i]
                if e is None:
                    continue
                assert e['image_id'] == ids[i] and e['category_id'] == (k + 1 if use_cats else -1)
                di = np.asarray(e['dtIds'], dtype=np.int64) - 1
                gi = np.asarray(e['gtIds'], dtype=np.int64) - 1
                rank[di] = np.arange(len(di))
                m = e['dtMatches'].astype(np.int64)
                match[di, a, :] = np.where(m > 0, m - 1 - first_gt[e['image_id']], -1).T
                ignore[di, a, :] = np.asarray(e['dtIgnore']).astype(np.uint8).T
                gt_ignore[gi, a] = np.asarray(e['gtIgnore']).astype(np.uint8)
                npig[k, a] += int((np.asarray(e['gtIgnore']) == 0).sum())
    assert rank.max(initial=0) < 1024 and match.max(initial=0) < 1024
    out = {'rank': rank.astype(np.int16), 'match': match.astype(np.int16), 'ignore': ignore, 'gt_ignore': gt_ignore, 'npig': npig,
           'precision': E.eval['precision'],
           'recall': E.eval['recall'], 'scores': E.eval['scores'], 'stats': np.asarray(E.stats, dtype=np.float64)}
    if not use_cats:                                                          # the order evaluateImg concatenates (cocoeval.py:245-247)
        do, go = [], []
        for im in images:
            i = im['image_id']
            do.append(np.asarray([d['id'] - 1 - first_dt[i] for c in E._paramsEval.catIds for d in E._dts[i, c]], dtype=np.int32))
            go.append(np.asarray([g['id'] - 1 - first_gt[i] for c in E._paramsEval.catIds for g in E._gts[i, c]], dtype=np.int32))
        out['dt_live'], out['gt_live'] = np.asarray([len(v) for v in do], np.int32), np.asarray([len(v) for v in go], np.int32)
        out['dt_order'] = np.concatenate(do) if do else np.zeros(0, np.int32)
        out['gt_order'] = np.concatenate(go) if go else np.zeros(0, np.int32)
    return out


def all_pairs_oks(coco_mod, eval_mod, images, area_rng):
    """computeOks of every (GT, detection) pair of every image: a run whose annotations all carry category 1, nothing cut"""
    E, _, _ = run(coco_mod, eval_mod, images, 1, area_rng, 'keypoints', max_dets=[100000], one_category=True)
    out = []
    for im in images:
        D, G = len(im['dt_score']), len(im['gt_cat'])
        if D == 0 or G == 0:
            continue
        o = np.asarray(E.ious[im['image_id'], 1])                            # [D in score order, G]
        inds = np.argsort([-float(s) for s in im['dt_score']], kind='mergesort')
        full = np.zeros((G, D))
        full[:, inds] = o.T
        out.append(full.reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


# ------------------------------------------------------------------------------------------------------------------ the sets
def person(rng, cx, cy, scale):
    """17 keypoints around (cx, cy): x, y rounded to one decimal"""
    return np.round(np.stack([cx + rng.uniform(-1, 1, KP) * scale, cy + rng.uniform(-1.5, 1.5, KP) * scale], 1), 1)


def kp_gt(xy, v, iscrowd=0, cat=1, num=None, area=None, box=None):
    """one GT row: keypoints [17, 3], num_keypoints (default: the count of v > 0), box (default: the extent of the points), area
    (default: w * h of the box), iscrowd, cat"""
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), (KP,))
    k = np.concatenate([np.asarray(xy, dtype=np.float64), v[:, None]], 1)
    if box is None:
        x0, y0 = k[:, 0].min(), k[:, 1].min()
        box = (x0, y0, k[:, 0].max() - x0, k[:, 1].max() - y0)
    return {'kps': k, 'num': int((v > 0).sum()) if num is None else num, 'box': tuple(float(b) for b in box),
            'area': float(box[2] * box[3]) if area is None else float(area), 'iscrowd': iscrowd, 'cat': cat}


def kp_image(image_id, dets, gts):
    """dets: (xy [17, 2], score, cat); gts: kp_gt rows"""
    dk = np.zeros((len(dets), KP, 3), np.float32)
    for i, d in enumerate(dets):
        dk[i, :, :2], dk[i, :, 2] = np.asarray(d[0], dtype=np.float32), 1.0
    return {'image_id': image_id, 'dt_kps': dk, 'dt_score': np.asarray([d[1] for d in dets], np.float32),
            'dt_cat': np.asarray([d[2] for d in dets], np.int32),
            'gt_kps': np.stack([g['kps'] for g in gts]) if gts else np.zeros((0, KP, 3)),
            'gt_num_kps': np.asarray([g['num'] for g in gts], np.int32),
            'gt_xywh': np.asarray([g['box'] for g in gts], np.float64).reshape(-1, 4),
            'gt_area': np.asarray([g['area'] for g in gts], np.float64), 'gt_iscrowd': np.asarray([g['iscrowd'] for g in gts], np.uint8),
            'gt_cat': np.asarray([g['cat'] for g in gts], np.int32)}


def jitter(rng, xy, scale):
    """detection points: the GT's plus noise, on the quarter-pixel grid the file stores them on"""
    return quarter(np.asarray(xy) + rng.normal(0, scale, (KP, 2)))


def quarter(xy):
    """onto the grid of 1/4 pixel: exact in float32, and stored as int16 quarters"""
    return (np.round(np.asarray(xy, dtype=np.float64) * 4) / 4).astype(np.float32)


def kp_rules_set(rng):
    ims = []
    # 90: a GT without visible keypoints (k1 == 0, box 100, 100, 40, 60): a detection inside its doubled box (OKS exactly 1), one outside
    g0 = kp_gt(person(rng, 120, 130, 15), 0, box=(100, 100, 40, 60), num=3)
    inside = quarter(np.stack([rng.uniform(70, 170, KP), rng.uniform(50, 210, KP)], 1))
    outside = inside + np.array([150.0, 0.0])
    ims.append(kp_image(90, [(inside, .9, 1), (outside, .8, 1)], [g0]))
    # 80: num_keypoints == 0 although v is visible (ignored, yet scored over the visible points); the reverse (not ignored, k1 == 0)
    p1, p2 = person(rng, 100, 100, 30), person(rng, 400, 200, 30)
    ims.append(kp_image(80, [(jitter(rng, p1, 2), .9, 1), (jitter(rng, p2, 2), .7, 1)],
                        [kp_gt(p1, 2, num=0), kp_gt(p2, 0, num=5)]))
    # 70: a crowd GT matched twice, a regular GT beside it
    p1, p2 = person(rng, 200, 200, 40), person(rng, 600, 200, 40)
    ims.append(kp_image(70, [(jitter(rng, p1, 3), .9, 1), (jitter(rng, p1, 4), .8, 1), (jitter(rng, p2, 3), .7, 1)],
                        [kp_gt(p1, 2, iscrowd=1), kp_gt(p2, 1)]))
    # 60: a GT of area 0 (e = d^2 / vars / 2.2e-16 / 2: exp underflows to 0 unless the points coincide); a detection ON its points
    p1 = np.round(person(rng, 300, 300, 20) * 2) / 2                          # halves: the float32 detection stands exactly on them
    ims.append(kp_image(60, [(p1, .6, 1), (jitter(rng, p1, 1), .5, 1)], [kp_gt(p1, 2, area=0.0)]))
    # 50, 40, 30: detections only, GTs only, nothing
    ims.append(kp_image(50, [(quarter(person(rng, 50, 50, 10)), .5, 1)], []))
    ims.append(kp_image(40, [], [kp_gt(person(rng, 50, 50, 10), 2)]))
    ims.append(kp_image(30, [], []))
    # 20: 25 detections (ranks past the cut at 20), tied scores; GT areas exactly 32^2 and 96^2
    pa, pb = person(rng, 200, 200, 12), person(rng, 600, 300, 40)
    gts = [kp_gt(pa, 2, area=32.0 ** 2), kp_gt(pb, 2, area=96.0 ** 2)]
    dets = [(jitter(rng, pa if j % 2 else pb, 1.5 + 0.4 * j), np.round(0.3 + 0.05 * (j % 6), 2), 1) for j in range(25)]
    ims.append(kp_image(20, dets, gts))
    return ims


def kp_random_set(rng, n_images=60, K=2):
    ims = []
    for i in range(n_images):
        gts, dets = [], []
        for _ in range(rng.randint(0, 6)):
            scale = np.exp(rng.uniform(np.log(8), np.log(80)))
            p = person(rng, rng.uniform(100, 900), rng.uniform(100, 400), scale)
            v = np.zeros(KP) if rng.rand() < 0.2 else rng.randint(0, 3, KP).astype(np.float64)
            g = kp_gt(p, v, iscrowd=int(rng.rand() < 0.1), cat=int(rng.randint(1, K + 1)))
            g['area'] = g['area'] * rng.choice([0.5, 0.8])
            gts.append(g)
            for _ in range(rng.randint(0, 9)):
                s = rng.choice([0.03, 0.12, 0.4]) * scale
                cat = g['cat'] if rng.rand() < 0.85 else int(rng.randint(1, K + 1))
                dets.append((jitter(rng, p, s), np.round(rng.uniform(0.05, 1.0), 2), cat))
        ims.append(kp_image(500 + int(rng.randint(0, 1000)) * 60 + (n_images - i), dets, gts))
    return ims


def kp_blocks_set(rng):
    """the OKS kernel's edges: one workgroup per (image, GT, 256 detection slots)"""
    ims = []
    for j, (D, G) in enumerate(((1, 1), (255, 1), (256, 1), (257, 1), (3, 12), (70, 5))):
        gts, centre = [], []
        for g in range(G):
            p = person(rng, 100 + 60 * g, 200, 25)
            gts.append(kp_gt(p, 0 if g == 3 else rng.randint(0, 3, KP).astype(np.float64) + (np.arange(KP) == 0)))
            centre.append(p)
        dets = [(jitter(rng, centre[d % G], rng.choice([1.0, 4.0, 15.0])), np.round(rng.uniform(0.05, 1.0), 3), 1) for d in range(D)]
        ims.append(kp_image(11 + 7 * j, dets, gts))
    return ims


def nocat_rules_set():
    image = base.image
    ims = []
    # 9: equal scores across categories, the higher category GIVEN first: the reference lists the category-2 detection ahead
    ims.append(image(9, [(10, 10, 30, 30, .8, 3), (11, 11, 31, 31, .8, 2), (100, 100, 150, 150, .8, 1)],
                     [(10, 10, 20, 20, 0, 3), (100, 100, 50, 50, 0, 2)]))
    # 8: two GTs of different categories with equal IoU 80 / 120 to one detection, the higher category given first: the later one
    # IN CATEGORY ORDER wins
    ims.append(image(8, [(10, 10, 20, 20, 1.0, 1)], [(12, 10, 10, 10, 0, 3), (8, 10, 10, 10, 0, 1)]))
    # 7: a crowd in one category (matched twice), a regular GT in another
    ims.append(image(7, [(12, 12, 30, 30, .9, 2), (20, 20, 35, 35, .8, 1), (100, 100, 140, 140, .7, 3)],
                     [(10, 10, 50, 50, 1, 3), (100, 100, 40, 40, 0, 1)]))
    # 6: a detection and a GT of a category outside 1..K take no part
    ims.append(image(6, [(0, 0, 10, 10, .9, 7), (0, 0, 10, 10, .6, 2)], [(0, 0, 10, 10, 0, 7), (0, 0, 10, 12, 0, 1)]))
    # 5, 4: GTs only, nothing
    ims.append(image(5, [], [(5, 5, 55, 55, 0, 2)]))
    ims.append(image(4, [], []))
    return ims


def nocat_xyxy_set():
    """hand-made proposals for the reference's 'proposal' reading of [x1, y1, x2, y2] as xywh: in image 3 the box (10, 10, 30, 30)
    covers its GT (10, 10, 20, 20) exactly when w = x2 - x1, but read as w = 30, h = 30 its IoU is 400 / 900 and the match is lost;
    in image 2 the box starts at the origin, where both readings agree, and the match stays"""
    image = base.image
    return [image(3, [(10, 10, 30, 30, .9, 1), (200, 100, 20, 10, .5, 1)], [(10, 10, 20, 20, 0, 1), (200, 100, 20, 10, 0, 1)]),
            image(2, [(0, 0, 10, 10, .8, 1)], [(0, 0, 10, 10, 0, 1)])]


def nocat_props_set(rng):
    """proposals: every category 1; 1010 in one image (ranks past 1000), 300 x 12 (an IoU block beyond the LDS stage), none"""
    def props(image_id, n, G):
        gx, gy = rng.uniform(0, 600, G), rng.uniform(0, 300, G)
        gw, gh = rng.uniform(20, 200, G), rng.uniform(20, 150, G)
        gts = [(np.round(gx[g], 1), np.round(gy[g], 1), np.round(gw[g], 1), np.round(gh[g], 1), int(g == 1), 1) for g in range(G)]
        dets = []
        for _ in range(n):
            g = gts[rng.randint(G)]
            s = rng.choice([0.05, 0.2, 0.5])
            x1, y1 = g[0] + rng.normal(0, s) * g[2], g[1] + rng.normal(0, s) * g[3]
            x2, y2 = x1 + g[2] * np.exp(rng.normal(0, s)), y1 + g[3] * np.exp(rng.normal(0, s))
            dets.append(tuple(float(v) for v in quarter([x1, y1, x2, y2])) + (np.round(rng.uniform(0.001, 1.0), 3), 1))
        return base.image(image_id, dets, gts)
    return [props(31, 1010, 5), props(17, 300, 12), props(23, 0, 3), props(5, 40, 2)]


def store_kp(out, name, images, K, area_rng, rec):
    cat = lambda key, dt: (np.concatenate([im[key] for im in images])).astype(dt)   # noqa: E731
    out[name + '_image_ids'] = np.asarray([im['image_id'] for im in images], dtype=np.int32)
    out[name + '_K'] = np.asarray(K, dtype=np.int32)
    out[name + '_area_rng'] = np.asarray(area_rng, dtype=np.float64)
    out[name + '_dt_counts'] = np.asarray([len(im['dt_score']) for im in images], dtype=np.int32)
    out[name + '_gt_counts'] = np.asarray([len(im['gt_cat']) for im in images], dtype=np.int32)
    xy = cat('dt_kps', np.float32).reshape(-1, KP, 3)[:, :, :2].astype(np.float64) * 4
    assert np.array_equal(xy, np.round(xy)) and np.abs(xy).max(initial=0) < 32768
    out[name + '_dt_kps_q'] = xy.astype(np.int16)
    out[name + '_dt_scores'], out[name + '_dt_cats'] = cat('dt_score', np.float32), cat('dt_cat', np.int32)
    out[name + '_gt_kps'] = cat('gt_kps', np.float64).reshape(-1, KP, 3)
    out[name + '_gt_num_kps'] = cat('gt_num_kps', np.int32)
    out[name + '_gt_boxes'] = cat('gt_xywh', np.float64).reshape(-1, 4)
    out[name + '_gt_areas'], out[name + '_gt_iscrowd'] = cat('gt_area', np.float64), cat('gt_iscrowd', np.uint8)
    out[name + '_gt_cats'] = cat('gt_cat', np.int32)
    for k, v in rec.items():
        out[name + '_' + k] = v


def check_margin(name, images, oks_flat, iou_thrs, sigmas):
    """the MARGIN CONDITION of the module's docstring"""
    var = (sigmas * 2) ** 2
    thr_gap, pair_gap, at = np.inf, np.inf, 0
    for im in images:
        D, G = len(im['dt_score']), len(im['gt_cat'])
        if D == 0 or G == 0:
            continue
        o = oks_flat[at:at + D * G].reshape(G, D)
        at += D * G
        thr_gap = min(thr_gap, np.abs(o[:, :, None] - iou_thrs[None, None, :]).min())
        d64 = im['dt_kps'].astype(np.float64)
        for d in range(D):
            cand = [g for g in range(G) if o[g, d] >= 0.5 - MARGIN]
            for i, g in enumerate(cand):
                for h in cand[i + 1:]:
                    e1 = knp.oks_terms(d64[d], im['gt_kps'][g], im['gt_xywh'][g], im['gt_area'][g], var)
                    e2 = knp.oks_terms(d64[d], im['gt_kps'][h], im['gt_xywh'][h], im['gt_area'][h], var)
                    if e1.tobytes() == e2.tobytes():
                        continue
                    pair_gap = min(pair_gap, abs(o[g, d] - o[h, d]))
    assert at == len(oks_flat)
    assert thr_gap > MARGIN and pair_gap > MARGIN, (name, thr_gap, pair_gap)
    print(name, "margin: closest threshold %.3g, smallest candidate gap %.3g, pairs %d" % (thr_gap, pair_gap, len(oks_flat)))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SCDA_REFERENCE", "/root/reference")
    kparams = knp.default_params()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        standin = base.make_standin(base.load_maskapi(ref_root, tmp))
        coco_mod, eval_mod = base.import_reference(ref_root, standin)
        P = eval_mod.Params('keypoints')
        assert np.array_equal(P.iouThrs, kparams['iou_thrs']) and np.array_equal(P.recThrs, kparams['rec_thrs'])
        assert P.maxDets == kparams['max_dets'] and np.array_equal(np.asarray(P.areaRng, dtype=np.float64), kparams['area_rng'])
        A3 = kparams['area_rng']

        # ---- the keypoint sets
        for name, K, ims in (('kp_rules', 1, kp_rules_set(np.random.RandomState(2021))),
                             ('kp_random', 2, kp_random_set(np.random.RandomState(2022))),
                             ('kp_blocks', 1, kp_blocks_set(np.random.RandomState(2023)))):
            E, fd, fg = run(coco_mod, eval_mod, ims, K, A3, 'keypoints')
            r = record(E, ims, fd, fg, K)
            r['oks'] = all_pairs_oks(coco_mod, eval_mod, ims, A3)
            check_margin(name, ims, r['oks'], kparams['iou_thrs'], kparams['sigmas'])
            store_kp(out, name, ims, K, A3, r)
            print(name, "stats", np.round(r['stats'], 4), "gts", sum(len(im['gt_cat']) for im in ims), "dets", len(r['rank']))
            if name == 'kp_rules':
                first = dict(zip([im['image_id'] for im in ims], np.concatenate([[0], np.cumsum(out[name + '_dt_counts'])])))
                gfirst = dict(zip([im['image_id'] for im in ims], np.concatenate([[0], np.cumsum(out[name + '_gt_counts'])])))
                o90 = r['oks'][:2]
                assert o90[0] == 1.0 and 0.0 <= o90[1] < 0.5, o90
                assert r['gt_ignore'][gfirst[80]].all() and not r['gt_ignore'][gfirst[80] + 1, 0], "num_keypoints decides the ignore flag"
                assert r['match'][first[80], 0, 0] == 0 and r['ignore'][first[80], 0, 0] == 1
                assert r['match'][first[70], 0, 0] == 0 and r['match'][first[70] + 1, 0, 0] == 0, "the crowd GT takes two detections"
                o60 = r['oks'][2 + 4 + 6:2 + 4 + 6 + 2]
                assert o60[0] == 1.0 and o60[1] == 0.0, o60
                assert r['gt_ignore'][gfirst[20]].tolist() == [0, 0, 1] and r['gt_ignore'][gfirst[20] + 1].tolist() == [0, 0, 0]
                rk = r['rank'][first[20]:first[20] + 25]
                assert rk.max() == 19 and (rk == -1).sum() == 5
                sc = out[name + '_dt_scores'][first[20]:first[20] + 25]
                assert len(np.unique(sc)) < len(sc)
            if name == 'kp_random':
                assert (r['stats'] > -1).all(), r['stats']
                k1 = (out[name + '_gt_kps'][:, :, 2] > 0).sum(1)
                assert (k1 == 0).any() and (out[name + '_gt_iscrowd'] == 1).any() and (out[name + '_dt_counts'] == 0).any()
            if name == 'kp_blocks':
                assert out[name + '_dt_counts'].tolist()[:4] == [1, 255, 256, 257] and out[name + '_gt_counts'].max() == 12

        # ---- useCats = 0: class rows
        params = cnp.default_params()
        ims = nocat_rules_set()
        E, fd, fg = run(coco_mod, eval_mod, ims, 3, params['area_rng'], 'bbox', use_cats=False)
        r = record(E, ims, fd, fg, 3, use_cats=False)
        base.store(out, 'nocat_rules', ims, 3, params['area_rng'], dict(r))
        out['nocat_rules_max_dets'] = np.asarray(params['max_dets'], np.int32)
        assert r['dt_order'][:3].tolist() == [2, 1, 0] and r['rank'][:3].tolist() == [2, 1, 0], "ties: category ascending"
        assert r['match'][3, 0, 0] == 0, "equal IoU: the later GT in category order wins"
        assert r['match'][4, 0, 0] == 0 and r['match'][5, 0, 0] == 0, "the crowd of another category takes two detections"
        assert r['dt_live'].tolist() == [3, 1, 3, 1, 0, 0] and r['gt_live'].tolist() == [2, 2, 2, 1, 1, 0]
        assert r['precision'].shape[2] == 1
        print("nocat_rules stats", np.round(r['stats'], 4))

        # ---- useCats = 0: proposals, as the reference's 'proposal' run scores them ([x1, y1, x2, y2] handed over as xywh)
        ims = nocat_props_set(np.random.RandomState(2024))
        E, fd, fg = run(coco_mod, eval_mod, ims, 1, params['area_rng'], 'bbox', max_dets=[1, 100, 1000], use_cats=False, xyxy_as_xywh=True)
        r = record(E, ims, fd, fg, 1, use_cats=False)
        base.store(out, 'nocat_props', ims, 1, params['area_rng'], dict(r))
        out['nocat_props_max_dets'] = np.asarray([1, 100, 1000], np.int32)
        assert (r['rank'][:1010] == -1).sum() == 10 and r['rank'][:1010].max() == 999
        assert tuple(r['precision'].shape) == (10, 101, 1, 4, 3), r['precision'].shape
        print("nocat_props stats", np.round(r['stats'], 4))

        # ---- useCats = 0: hand-made proposals under the same reading
        ims = nocat_xyxy_set()
        E, fd, fg = run(coco_mod, eval_mod, ims, 1, params['area_rng'], 'bbox', max_dets=[1, 100, 1000], use_cats=False, xyxy_as_xywh=True)
        r = record(E, ims, fd, fg, 1, use_cats=False)
        base.store(out, 'nocat_xyxy', ims, 1, params['area_rng'], dict(r))
        out['nocat_xyxy_max_dets'] = np.asarray([1, 100, 1000], np.int32)
        assert r['match'][0, 0, 0] == -1, "(x2, y2) read as (w, h) loses the match of a box that covers its GT"
        assert r['match'][1, 0, 0] == 1, "a box handed over as (x, y, w, h) by chance (x2, y2 = its size) keeps it"
        assert r['match'][2, 0, :].tolist() == [0] * 10, "at the origin both readings agree"
        print("nocat_xyxy stats", np.round(r['stats'], 4))

        # ---- useCats = 0: 'segm' over random_segm's planes of coco_eval_ref.npz
        z = dict(np.load(os.path.join(HERE, "coco_eval_ref.npz")))
        simgs, K, sparams = cnp.load_set(z, 'random_segm')
        h, w = (int(v) for v in z['random_segm_size'])
        unpack = lambda bits: np.unpackbits(bits.view(np.uint8), axis=-1, bitorder='little').astype(bool)[:, :h, :w]   # noqa: E731
        for im in simgs:
            im['dt_mask'], im['gt_mask'] = list(unpack(z['random_segm_dt_bits'][im['dt']])), list(unpack(z['random_segm_gt_bits'][im['gt']]))
        E, fd, fg = run(coco_mod, eval_mod, simgs, K, sparams['area_rng'], 'segm', size=(h, w), use_cats=False)
        r = record(E, simgs, fd, fg, K, use_cats=False)
        for k, v in r.items():
            out['nocat_segm_' + k] = v
        assert (r['stats'] > -1).all(), r['stats']
        print("nocat_segm stats", np.round(r['stats'], 4))
    path = os.path.join(HERE, "coco_kps_ref.npz")
    for k in [k for k in out if k.startswith('nocat_') and k.endswith('_dt_areas')]:
        del out[k]                                                            # (the loaders compute the areas from the corners)
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member date, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main()
