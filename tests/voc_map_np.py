"""The Cityscapes mAP rules R1..R4 of include/scda_ops.h restated in numpy (the reference: validate()'s rows, utils/cal_mAP.py,
bbox_helper.compute_recall).  Used by the tests of scda_amd/map_eval.py and by tests/golden/make_golden_voc_map.py, which asserts it
against the reference's own code.  An image is a dict: 'name', 'det' float32 [n, 7] = (b, x1, y1, x2, y2, score, class) (the live rows,
in the given order), 'info' float32 [k] = (h, w, ..., scale), 'gt' int32 [g, 5] = (x1, y1, x2, y2, label) in meta order (empty when the
meta has no such image); for the recall also 'props' float32 [p, 6] (live rows) and 'rgts' float32 [r, >= 4]."""
import numpy as np


def image_rows(det, info, num_classes, keep_num=100, scale_column=-1):
    """R1 -> {'rank' [n], 'kept' bool [n], 'box' int32 [n, 4], 'score' f32 [n], 'cls' [n], 'order': the kept rows in file order (class
    ascending, then rank)}"""
    det = np.asarray(det, dtype=np.float32).reshape(-1, 7)
    info = np.asarray(info, dtype=np.float32)
    n = len(det)
    by_score = np.argsort(-det[:, 5].astype(np.float64), kind='stable')      # float32 -> float64 is exact: the float32 order, ties earlier first
    rank = np.empty(n, dtype=np.int64)
    rank[by_score] = np.arange(n)
    cls = det[:, 6].astype(np.int64)
    kept = (rank < keep_num) & (cls >= 1) & (cls <= num_classes - 1)
    h, w, scale = info[0], info[1], info[scale_column]
    one, zero = np.float32(1), np.float32(0)
    box = np.empty((n, 4), dtype=np.float32)
    for col, hi in ((0, w - one), (1, h - one), (2, w - one), (3, h - one)):
        box[:, col] = np.minimum(np.maximum(det[:, 1 + col], zero), hi) / scale
    assert box.dtype == np.float32
    order = sorted(np.nonzero(kept)[0], key=lambda d: (cls[d], rank[d]))
    return {'rank': rank, 'kept': kept, 'box': np.trunc(box).astype(np.int32), 'score': det[:, 5].copy(), 'cls': cls,
            'order': np.asarray(order, dtype=np.int64)}


def best_iou(box, gts):
    """calIoU: (best, index) over gts int [m, 4] in order; (-1, -1) when nothing overlaps strictly"""
    x1, y1, x2, y2 = (int(v) for v in box)
    best, which = -1, -1
    for k, g in enumerate(gts):
        gx1, gy1, gx2, gy2 = (int(v) for v in g[:4])
        ix1, iy1, ix2, iy2 = max(x1, gx1), max(y1, gy1), min(x2, gx2), min(y2, gy2)
        if ix1 < ix2 and iy1 < iy2:
            inter = (ix2 - ix1 + 1) * (iy2 - iy1 + 1)
            iou = inter / ((x2 - x1 + 1) * (y2 - y1 + 1) + (gx2 - gx1 + 1) * (gy2 - gy1 + 1) - inter)    # Python ints, one double division
            if iou > best:
                best, which = iou, k
    return best, which


def match_image(rows, gt, num_classes, iou_thr=0.5):
    """R2 -> tp int [n], match int [n] (the claimed ground truth's row of the image, -1), claimed int [g]"""
    gt = np.asarray(gt, dtype=np.int64).reshape(-1, 5)
    n = len(rows['rank'])
    tp, match, claimed = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.zeros(len(gt), dtype=np.int32)
    for c in range(1, num_classes):
        gl = np.nonzero(gt[:, 4] == c)[0]
        for d in rows['order'][rows['cls'][rows['order']] == c]:             # the class's kept rows in rank order
            best, which = best_iou(rows['box'][d], gt[gl])
            if which >= 0 and best >= iou_thr and not claimed[gl[which]]:
                tp[d], match[d], claimed[gl[which]] = 1, gl[which], 1
    return tp, match, claimed


def accumulate(per_image, num_classes, sum_gt):
    """R3 over [(rows, tp)] in the order the images were added -> ap, max_recall float64 [C], rows int [C]"""
    ap, max_recall, nrows = np.zeros(num_classes), np.zeros(num_classes), np.zeros(num_classes, dtype=np.int32)
    for c in range(1, num_classes):
        score, hit = [], []
        for rows, tp in per_image:
            for d in rows['order']:
                if rows['cls'][d] == c:
                    score.append(rows['score'][d]); hit.append(tp[d])
        n = len(score)
        nrows[c] = n
        if n == 0:
            continue                                                         # the reference raises ValueError here
        by_score = np.argsort(-np.asarray(score, dtype=np.float64), kind='stable')
        hit = np.asarray(hit, dtype=np.float64)[by_score]
        tp, fp = np.cumsum(hit), np.cumsum(1.0 - hit)
        with np.errstate(divide='ignore', invalid='ignore'):
            rec = tp / np.float64(sum_gt[c])
            prec = tp / (tp + fp)
            env = np.maximum.accumulate(prec[::-1])[::-1]
            a = np.float64(0.0)
            for v in range(n):
                a = a + (rec[v] * env[v] if v == 0 else (rec[v] - rec[v - 1]) * env[v])
            ap[c], max_recall[c] = a, np.max(rec)
    return ap, max_recall, nrows


def overlaps_f32(gts, props):
    """scda_bbox_overlaps_hip's float32 rule: gts [r, >= 4] x props [p, >= 4] -> [r, p]"""
    g, q = np.asarray(gts, dtype=np.float32)[:, None, :4], np.asarray(props, dtype=np.float32)[None, :, :4]
    iw = np.minimum(g[..., 2], q[..., 2]) - np.maximum(g[..., 0], q[..., 0])
    ih = np.minimum(g[..., 3], q[..., 3]) - np.maximum(g[..., 1], q[..., 1])
    ua = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1]) + (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1]) - iw * ih
    assert ua.dtype == np.float32
    hit = (iw > 0) & (ih > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(hit, (iw * ih) / np.where(hit, ua, np.float32(1)), np.float32(0))


def recall(props, rgts):
    """R4 -> (recalled, rows given); props: the live proposals [p, >= 5] (columns 1..4)"""
    rgts = np.asarray(rgts, dtype=np.float32)
    if len(props) == 0 or len(rgts) == 0:
        return 0, len(rgts)
    return int((overlaps_f32(rgts, np.asarray(props)[:, 1:5]).max(axis=1) > np.float32(0.5)).sum()), len(rgts)


def evaluate(images, num_classes, sum_gt=None, iou_thr=0.5, keep_num=100, scale_column=-1):
    """every rule over the images in order -> {'per_image': [{rows..., 'tp', 'match', 'claimed'}], 'ap', 'max_recall', 'rows', 'sum_gt',
    'mAP', 'rpn_recalled', 'rpn_gts'}"""
    per, counted = [], np.zeros(num_classes, dtype=np.int64)
    rc = ng = 0
    for im in images:
        rows = image_rows(im['det'], im['info'], num_classes, keep_num, scale_column)
        gt = np.asarray(im['gt'], dtype=np.int64).reshape(-1, 5)
        tp, match, claimed = match_image(rows, gt, num_classes, iou_thr)
        lab = gt[:, 4]
        counted += np.bincount(lab[(lab >= 1) & (lab < num_classes)], minlength=num_classes)[:num_classes]
        per.append(dict(rows, tp=tp, match=match, claimed=claimed))
        if 'props' in im:
            r, g = recall(im['props'], im['rgts'])
            rc, ng = rc + r, ng + g
    total = counted if sum_gt is None else np.asarray(sum_gt)
    ap, max_recall, nrows = accumulate([(e, e['tp']) for e in per], num_classes, total)
    return {'per_image': per, 'ap': ap, 'max_recall': max_recall, 'rows': nrows, 'sum_gt': np.asarray(total, dtype=np.int64),
            'mAP': np.mean(ap[1:]), 'rpn_recalled': rc, 'rpn_gts': ng}


def parse_text_rows(text):
    """results rows `name x1 y1 x2 y2 score class` -> images in order of first appearance: [{'name', 'det' float32 [n, 7]}], the rows
    of an image in file order, the coordinates parsed back to float32"""
    names, dets = [], {}
    for line in text.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] not in dets:
            names.append(f[0]); dets[f[0]] = []
        dets[f[0]].append([0.0] + [float(v) for v in f[1:7]])
    return [{'name': k, 'det': np.asarray(dets[k], dtype=np.float32).reshape(-1, 7)} for k in names]


# ---- the fixture's layout (tests/golden/voc_map_ref.npz), per set s: flat arrays cut by the per-image counts
def load_set(z, s):
    """-> (images, num_classes, sum_gt or None)"""
    names = [str(v) for v in z[s + '_names']]
    dc, gc = z[s + '_det_counts'], z[s + '_gt_counts']
    d0, g0 = np.concatenate([[0], np.cumsum(dc)]), np.concatenate([[0], np.cumsum(gc)])
    has_recall = s + '_props' in z
    if has_recall:
        pc, rcn = z[s + '_prop_counts'], z[s + '_rgt_counts']
        p0, r0 = np.concatenate([[0], np.cumsum(pc)]), np.concatenate([[0], np.cumsum(rcn)])
    images = []
    for i, name in enumerate(names):
        im = {'name': name, 'det': z[s + '_det'][d0[i]:d0[i + 1]], 'info': z[s + '_info'][i], 'gt': z[s + '_gt'][g0[i]:g0[i + 1]],
              'dt': slice(d0[i], d0[i + 1]), 'gts': slice(g0[i], g0[i + 1])}
        if has_recall:
            im['props'], im['rgts'] = z[s + '_props'][p0[i]:p0[i + 1]], z[s + '_rgts'][r0[i]:r0[i + 1]]
        images.append(im)
    return images, int(z[s + '_C']), (z[s + '_sum_gt'] if s + '_sum_gt' in z else None)
