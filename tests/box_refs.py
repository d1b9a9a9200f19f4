"""Plain numpy restatements of the box logic between the networks (detection_ops.hip's NMS, box_ops.hip, infer_ops.hip) and the
builders of the structured inputs that tests/test_box_refs.py (CPU) and tests/test_box_edges_gpu.py (MI355X) share.  numpy only,
no device, no C oracle: every function is the box-by-box / row-by-row statement of one operation, in the dtypes the kernels'
comments state, so that a kernel and its restatement agree BIT FOR BIT (integers, copied floats, single IEEE operations).
tests/test_box_refs.py pins every restatement to this repository's numpy path, the C oracle and the reference's golden vectors."""
import numpy as np

from nms_cases import iou_rows_f32

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- NMS ----------
def nms_greedy(boxes, thresh, valid=None, max_keep=0):
    """the O(n^2) greedy sweep, box by box: float32 IoU(+1) in the operation order of nms_cases.iou_rows_f32, suppression on a
    strict >, invalid boxes are neither kept nor suppress anything, indices into the ORIGINAL list, stops after max_keep kept"""
    b = np.ascontiguousarray(boxes, dtype=F)
    n, t = b.shape[0], F(thresh)
    removed = np.zeros(n, dtype=bool) if valid is None else ~np.asarray(valid).astype(bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if max_keep > 0 and len(keep) >= max_keep:
            break
        if i + 1 < n:
            js = np.arange(i + 1, n)
            removed[js[iou_rows_f32(b, i, js) > t]] = True
    return np.array(keep, dtype=np.int64)


def nms_mask_np(boxes, thresh):
    """uint64 [n, ceil(n/64)]: bit j of row i's words = (j > i and IoU(i, j) > thresh) -- the upper triangle the sweep reads"""
    b = np.ascontiguousarray(boxes, dtype=F)
    n, t = b.shape[0], F(thresh)
    m = np.zeros((n, (n + 63) // 64), dtype=np.uint64)
    for i in range(n - 1):
        js = np.arange(i + 1, n)
        for j in js[iou_rows_f32(b, i, js) > t]:
            m[i, j // 64] |= np.uint64(1) << np.uint64(j % 64)
    return m


def _scored(b):
    """[n,4] -> float32 [n,5] with strictly decreasing scores (the kernels take score-sorted lists; NMS never reads the score)"""
    n = b.shape[0]
    s = (n - np.arange(n)) / float(n + 1)
    return np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64), s[:, None]], 1).astype(F))


def chain_boxes(n, step=10, width=40, height=20, x0=0, y0=0):
    """box i = [x0 + step*i, y0, x0 + step*i + width - 1, y0 + height - 1].  With the defaults the IoU(+1) of neighbours is
    30*20 / (2*800 - 600) = 0.6 and of next-neighbours 400 / 1200 = 0.333: at thresh 0.5 box i suppresses only box i + 1, so the
    keep list is the even indices and a 64-box chunk needs 64 fixpoint rounds.  width = 60: neighbours 0.714, next-neighbours
    800 / 1600 = 0.5, third neighbours 0.333 (a two-step chain at thresh 0.45: every third box is kept)"""
    i = np.arange(n, dtype=np.float64)
    return _scored(np.stack([x0 + step * i, y0 + 0 * i, x0 + step * i + width - 1, y0 + height - 1 + 0 * i], 1))


def disjoint_grid(n, cols=16, size=10, pitch=16, x0=0, y0=0):
    """n boxes of size x size pixels on a pitch-spaced grid: no two overlap, NMS keeps every one"""
    i = np.arange(n)
    x, y = x0 + (i % cols) * float(pitch), y0 + (i // cols) * float(pitch)
    return _scored(np.stack([x, y, x + size - 1, y + size - 1], 1))


def exact_threshold_pairs(n_pairs, lead=0, thresh=0.5):
    """`lead` disjoint boxes, then n_pairs pairs (A, B) far from each other whose float32 IoU(+1) equals float32(thresh) exactly:
    thresh 0.5: A = [x,0,x+9,9] (100 px), B = [x,0,x+9,19] (200 px), 100/200; thresh 0.7: B = [x,0,x+6,9] (70 px) inside A, 70/100
    (a correctly rounded float32 division of 7 by 10 IS float32(0.7)).  Strict > keeps B.  lead = 1 puts a pair across every
    chunk boundary (positions 63|64, 127|128, ...)"""
    rows = [[1000.0 + 40 * k, 500, 1000.0 + 40 * k + 9, 509] for k in range(lead)]
    for p in range(n_pairs):
        x = 40.0 * p
        rows.append([x, 0, x + 9, 9])
        rows.append([x, 0, x + 9, 19] if thresh == 0.5 else [x, 0, x + 6, 9])
    assert thresh in (0.5, 0.7)
    return _scored(np.array(rows))


def duplicates(n):
    """n copies of one box: the first suppresses all"""
    return _scored(np.tile(np.array([[5.0, 7, 104, 86]]), (n, 1)))


def nms_structured_cases():
    """(name, boxes [n,5], thresh) of every structured NMS input of the edge tests"""
    out = [("chain_%d" % n, chain_boxes(n), 0.5) for n in (64, 65, 128, 255, 256, 257, 320, 511, 513)]
    out += [("chain2_%d" % n, chain_boxes(n, width=60), 0.45) for n in (64, 257)]
    out += [("chain2_at_threshold_257", chain_boxes(257, width=60), 0.5)]       # next-neighbours sit exactly ON the threshold
    out += [("first_suppresses_all_%d" % n, duplicates(n), 0.5) for n in (64, 300)]
    out += [("nothing_overlaps_%d" % n, disjoint_grid(n), 0.5) for n in (1, 257)]
    out += [("pairs_t05_lead%d" % k, exact_threshold_pairs(65, k, 0.5), 0.5) for k in (0, 1)]
    out += [("pairs_t07_lead%d" % k, exact_threshold_pairs(65, k, 0.7), 0.7) for k in (0, 1)]
    return out


def segment_lists():
    """(lists, thresh): score-sorted lists of lengths 0, 1, 64, 65, 256, 257 (and a second empty one) mixing chains and disjoint boxes"""
    def mixed(n):      # a chain, then disjoint boxes far from it, then a second chain
        a = n // 3
        return _scored(np.vstack([chain_boxes(a)[:, :4], disjoint_grid(n - 2 * a, y0=100)[:, :4], chain_boxes(a, y0=2000)[:, :4]]))
    lists = [np.zeros((0, 5), F), chain_boxes(1), chain_boxes(64), mixed(65), np.zeros((0, 5), F), mixed(256), chain_boxes(257),
             disjoint_grid(64), exact_threshold_pairs(32, 1, 0.5)]
    return lists, 0.5


def segment_table(lists):
    """-> boxes [rows,5] (the lists back to back), seg int64 [S,3] = (first row, length, first mask word), max_n"""
    seg, row, word = [], 0, 0
    for b in lists:
        n = b.shape[0]
        seg.append((row, n, word))
        row += n
        word += n * ((n + 63) // 64)
    boxes = np.vstack(lists).astype(F) if row else np.zeros((0, 5), F)
    return np.ascontiguousarray(boxes), np.array(seg, dtype=np.int64).reshape(-1, 3), max(b.shape[0] for b in lists)


# ----------------------------------------------------------------------------------------------------- ranking rules ----------
def topk_stable(score, top_n):
    """RPN top-k: score descending, ties by ascending anchor index; top_n <= 0 or >= KA: all anchors (test_infer_rules.rank_topk)"""
    order = np.argsort(-score, kind='stable')
    return order if top_n <= 0 or top_n >= score.shape[0] else order[:top_n]


def rank_desc_later_first(score):
    """score descending, ties by DESCENDING position: a stable ascending sort, reversed (as in test_infer_rules.py)"""
    return np.argsort(score, kind='stable')[::-1]


def score_plane(kind, KA, seed):
    """float32 [KA] fg scores in [0, 1]: random / quantised to 3 levels / all equal / containing exact 0.0 and 1.0"""
    rs = np.random.RandomState(seed)
    s = rs.uniform(0.0, 1.0, KA).astype(F)
    if kind == "quant3":
        s = (np.floor(s * 3) / 3).astype(F)
    elif kind == "equal":
        s[:] = F(0.5)
    elif kind == "zero_one":
        s[rs.randint(0, KA, max(1, KA // 5))] = F(0.0)
        s[rs.randint(0, KA, max(1, KA // 5))] = F(1.0)
    else:
        assert kind == "random"
    return s


def prob_from_scores(s, A, fh, fw, bg=np.nan):
    """scores [B, KA] in anchor order k = (h*fw + w)*A + a -> prob [B, 2A, fh, fw]: fg of anchor a in channel 2a + 1; the bg
    channels hold `bg` (NaN: nothing may read them)"""
    B = s.shape[0]
    p = np.full((B, fh, fw, A, 2), bg, dtype=F)
    p[..., 1] = s.reshape(B, fh, fw, A)
    return np.ascontiguousarray(p.reshape(B, fh, fw, 2 * A).transpose(0, 3, 1, 2))


# --------------------------------------------------------------------------------------------------- box arithmetic ----------
def iou_f32(boxes, query):
    """float32 [n, m]: IoU without +1, 0 unless iw > 0 and ih > 0, one IEEE operation per operator in box_ops.hip's bbox_iou order:
    ua = (b2-b0)*(b3-b1) + (q2-q0)*(q3-q1) - iw*ih"""
    b = np.asarray(boxes, dtype=F)[:, None, :4]
    q = np.asarray(query, dtype=F)[None, :, :4]
    q_area = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])
    inter = iw * ih
    ua = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) + q_area - inter
    hit = (iw > 0) & (ih > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = inter / ua
    out = np.where(hit, v, F(0)).astype(F)
    assert out.dtype == F
    return out


def anchor_labels_np(anchors32, gts, neg, pos, min_gt_best):
    """functions/anchor_target.py:38-64 for ARBITRARY anchor arrays [KA,4] and gts [G,>=4] -> dict(labels int8 [KA], best_gt int32,
    best_iou float32, pos_list, neg_list (ascending), counts (n_pos, n_neg)).  Order of assignments: labels = -1; best_iou < neg
    -> 0; every (anchor, gt) pair whose IoU equals that gt's best (if that best >= min_gt_best) -> 1 and best_gt <- that gt, the
    pairs visited in np.where's row-major order, so the LAST such gt of an anchor wins; best_iou > pos -> 1.  Thresholds are
    compared in float32 (a float32 array against a Python float)."""
    iou = iou_f32(anchors32, gts)
    KA, G = iou.shape
    best_gt = iou.argmax(axis=1).astype(np.int32)                 # first maximum
    best_iou = iou[np.arange(KA), best_gt]
    per_gt = iou.max(axis=0).copy()
    per_gt[per_gt < F(min_gt_best)] = F(-1)
    labels = np.full(KA, -1, dtype=np.int8)
    labels[best_iou < F(neg)] = 0
    for k in np.where((iou == per_gt[None, :]).any(axis=1))[0]:
        for g in range(G):                                        # row-major: anchor by anchor, gt ascending
            if iou[k, g] == per_gt[g]:
                best_gt[k] = g
                labels[k] = 1
    labels[best_iou > F(pos)] = 1
    pos_list = np.where(labels > 0)[0].astype(np.int32)
    neg_list = np.where(labels == 0)[0].astype(np.int32)
    return dict(labels=labels, best_gt=best_gt, best_iou=best_iou, pos_list=pos_list, neg_list=neg_list,
                counts=np.array([pos_list.size, neg_list.size], dtype=np.int32))


def apply_drops(labels, pos_list, drop_pos, neg_list, drop_neg):
    """labels[list[drop]] = -1 for the surplus the host drew (indices INTO the lists)"""
    labels = labels.copy()
    if drop_pos is not None and len(drop_pos):
        labels[pos_list[np.asarray(drop_pos)]] = -1
    if drop_neg is not None and len(drop_neg):
        labels[neg_list[np.asarray(drop_neg)]] = -1
    return labels


def anchor_maps_np(labels, best_gt, anchors64, gts, A, fh, fw):
    """-> cls_targets int64 [A,fh,fw], loc_targets, loc_masks float32 [4A,fh,fw] (anchor k = (y*fw + x)*A + a).  Encode of
    utils/bbox_helper.py:70-86 in the reference's dtypes: the gt's centre / size in float32, the anchor's in float64, the
    quotient / log in float64, stored as float32"""
    KA = A * fh * fw
    assert labels.shape[0] == KA
    t = np.zeros((KA, 4), dtype=F)
    on = labels > 0
    g = np.asarray(gts, dtype=F)[best_gt[on]]
    r = np.asarray(anchors64, dtype=np.float64)[on]
    gcx, gcy, gw, gh = (g[:, 0] + g[:, 2]) / F(2), (g[:, 1] + g[:, 3]) / F(2), g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    assert gcx.dtype == F and gw.dtype == F
    rcx, rcy, rw, rh = (r[:, 0] + r[:, 2]) / 2., (r[:, 1] + r[:, 3]) / 2., r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    t[on, 0] = ((gcx.astype(np.float64) - rcx) / rw).astype(F)
    t[on, 1] = ((gcy.astype(np.float64) - rcy) / rh).astype(F)
    t[on, 2] = np.log(gw.astype(np.float64) / rw).astype(F)
    t[on, 3] = np.log(gh.astype(np.float64) / rh).astype(F)
    m = np.repeat(on.astype(F)[:, None], 4, 1)
    cls_t = labels.astype(np.int64).reshape(fh, fw, A).transpose(2, 0, 1)
    to_map = lambda a: a.reshape(fh, fw, A * 4).transpose(2, 0, 1)
    return np.ascontiguousarray(cls_t), np.ascontiguousarray(to_map(t)), np.ascontiguousarray(to_map(m))


def decode_np(anchors64, deltas32, exp_wh32, img_h, img_w, min_size):
    """utils/bbox_helper.py:88-110 + the size test of functions/rpn_proposal.py:57-58 on ranked candidates: float64 anchors, float32
    deltas promoted, exp_wh32 [n,2] = the float32 exponentials of the size deltas -> boxes float32 [n,4] (rounded once), ok bool [n]
    (tested on the float64 boxes)"""
    r = np.asarray(anchors64, dtype=np.float64)
    d = np.asarray(deltas32, dtype=F).astype(np.float64)
    e = np.asarray(exp_wh32, dtype=F).astype(np.float64)
    rcx, rcy, rw, rh = (r[:, 0] + r[:, 2]) / 2., (r[:, 1] + r[:, 3]) / 2., r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    cx, cy, w, h = d[:, 0] * rw + rcx, d[:, 1] * rh + rcy, e[:, 0] * rw, e[:, 1] * rh
    x1, y1, x2, y2 = cx - w / 2., cy - h / 2., cx + w / 2., cy + h / 2.
    x1, x2 = (np.minimum(np.maximum(v, 0.), float(img_w) - 1.) for v in (x1, x2))
    y1, y2 = (np.minimum(np.maximum(v, 0.), float(img_h) - 1.) for v in (y1, y2))
    ok = (x2 - x1 + 1. >= float(min_size)) & (y2 - y1 + 1. >= float(min_size))
    return np.stack([x1, y1, x2, y2], 1).astype(F), ok


def proposals_np(score, deltas32, anchors64, img_h, img_w, pre_nms_top_n, min_size, nms_thresh, post_nms_top_n, image_index,
                 order=None, exp_wh32=None):
    """functions/rpn_proposal.py:36-66 of ONE image: score [KA], deltas32 [KA,4] in anchor order -> float32 [kept, 6] rows
    (image, x1, y1, x2, y2, score).  order: the ranking (default: the stable top-k rule); exp_wh32: the float32 exponentials of the
    ranked size deltas (default: numpy's)"""
    if order is None:
        order = topk_stable(score, pre_nms_top_n)
    if exp_wh32 is None:
        exp_wh32 = np.exp(np.asarray(deltas32, dtype=F)[order, 2:4])
    boxes, ok = decode_np(np.asarray(anchors64)[order], np.asarray(deltas32)[order], exp_wh32, img_h, img_w, min_size)
    props = np.concatenate([boxes, np.asarray(score, dtype=F)[order][:, None]], 1)
    keep = nms_greedy(props, nms_thresh, valid=ok, max_keep=max(post_nms_top_n, 0))
    return np.concatenate([np.full((keep.size, 1), image_index, dtype=F), props[keep]], 1).astype(F)


def proposal_match_np(props, gts, img_h, img_w, pos, neg_hi, neg_lo):
    """functions/proposal_target.py:38-62: candidates = the proposals' boxes (columns 1..4) then the gt boxes, clipped to the image
    in float32 (np.clip on float32 columns against float32(img) - 1), IoU against every gt on the CLIPPED box, first maximum;
    label 1 = best_iou > pos, 0 = neg_lo <= best_iou < neg_hi and not 1, -1 = neither -> dict(rois float32 [n+G,4], best_iou,
    best_gt int32, labels int8, pos_list, neg_list, counts)"""
    props, gts = np.asarray(props, dtype=F), np.asarray(gts, dtype=F)
    cand = np.vstack([props[:, 1:5], gts[:, :4]]).astype(F)
    hi_x, hi_y = F(img_w) - F(1), F(img_h) - F(1)
    rois = cand.copy()
    rois[:, 0::2] = np.minimum(np.maximum(cand[:, 0::2], F(0)), hi_x)
    rois[:, 1::2] = np.minimum(np.maximum(cand[:, 1::2], F(0)), hi_y)
    iou = iou_f32(rois, gts)
    best_gt = iou.argmax(axis=1).astype(np.int32)
    best_iou = iou[np.arange(iou.shape[0]), best_gt]
    labels = np.where(best_iou > F(pos), 1, np.where((best_iou < F(neg_hi)) & (best_iou >= F(neg_lo)), 0, -1)).astype(np.int8)
    pos_list = np.where(labels > 0)[0].astype(np.int32)
    neg_list = np.where(labels == 0)[0].astype(np.int32)
    return dict(rois=rois, best_iou=best_iou, best_gt=best_gt, labels=labels, pos_list=pos_list, neg_list=neg_list,
                counts=np.array([pos_list.size, neg_list.size], dtype=np.int32))


def proposal_finalize_np(cand_rois, sel, gt_of, enc, gts, C, image_index):
    """the gather of functions/proposal_target.py:64-136 after the host drew the rows: sel [R] candidate indices, gt_of [R] matched gt
    (>= 0 foreground, label = that gt's class; -1 background, label 0), enc float32 [R,4] -> rois float32 [R,5], labels int64 [R],
    loc_targets, loc_weights float32 [R,4C] (the row's target / ones in the four columns of its class, zeros elsewhere)"""
    R = len(sel)
    rois = np.concatenate([np.full((R, 1), image_index, dtype=F), np.asarray(cand_rois, dtype=F)[np.asarray(sel)]], 1)
    labels = np.zeros(R, dtype=np.int64)
    t = np.zeros((R, 4 * C), dtype=F)
    w = np.zeros((R, 4 * C), dtype=F)
    for i in range(R):
        if gt_of[i] >= 0:
            lab = int(gts[gt_of[i], 4])
            labels[i] = lab
            t[i, 4 * lab:4 * lab + 4] = enc[i]
            w[i, 4 * lab:4 * lab + 4] = 1
    return rois, labels, t, w


def predict_np(rois, roi_counts, P, prob, loc, info, cfg):
    """functions/predict_bbox.py:13-66 (predict_by_rule of test_infer_rules.py) on fixed-capacity inputs: rois float32 [B*P,5], of
    which the first roi_counts[b] rows of image b are real, prob [B*P,C], loc [B*P,4C], info float32 [B,>=2] (h, w) -> det float32
    [B, top_n, 7] = (b, x1, y1, x2, y2, score, class), rows past the count zero, and the counts int32 [B].  Rows >= roi_counts[b]
    are never read."""
    C = prob.shape[1]
    stds, means = np.array(cfg['bbox_normalize_stds'], dtype=np.float64), np.array(cfg['bbox_normalize_means'], dtype=np.float64)
    thr, top_n = F(cfg['score_thresh']), cfg['top_n']
    B = len(roi_counts)
    det = np.zeros((B, top_n, 7), dtype=F)
    counts = np.zeros(B, dtype=np.int32)
    for b in range(B):
        m = min(int(roi_counts[b]), P)
        rows = []
        if m:
            ro = np.asarray(rois, dtype=F)[b * P:b * P + m, 1:5]
            rcx, rcy, rw, rh = (ro[:, 0] + ro[:, 2]) / F(2), (ro[:, 1] + ro[:, 3]) / F(2), ro[:, 2] - ro[:, 0], ro[:, 3] - ro[:, 1]
            assert rcx.dtype == F and rw.dtype == F                           # corner_to_center on float32 RoIs stays float32
            hi_x, hi_y = np.float64(F(info[b][1]) - F(1)), np.float64(F(info[b][0]) - F(1))   # float32 w - 1, as numpy's scalar
        for c in range(1, C if m else 1):
            d = np.asarray(loc, dtype=F)[b * P:b * P + m, 4 * c:4 * c + 4].astype(np.float64) * stds[None, :] + means[None, :]
            cx, cy = d[:, 0] * rw.astype(np.float64) + rcx.astype(np.float64), d[:, 1] * rh.astype(np.float64) + rcy.astype(np.float64)
            w, h = np.exp(d[:, 2]) * rw.astype(np.float64), np.exp(d[:, 3]) * rh.astype(np.float64)
            x1, y1, x2, y2 = cx - w / 2., cy - h / 2., cx + w / 2., cy + h / 2.
            x1, x2 = (np.minimum(np.maximum(v, 0.), hi_x) for v in (x1, x2))
            y1, y2 = (np.minimum(np.maximum(v, 0.), hi_y) for v in (y1, y2))
            s = np.asarray(prob, dtype=F)[b * P:b * P + m, c]
            bx = np.stack([x1, y1, x2, y2], 1).astype(F)
            if thr > 0:
                above = s > thr
                s, bx = s[above], bx[above]
            if s.size == 0:
                continue
            o = rank_desc_later_first(s)
            cand = np.concatenate([bx[o], s[o][:, None]], 1).astype(F)
            kept = cand[nms_greedy(cand, cfg['nms_iou_thresh'])]
            rows.append(np.concatenate([np.full((len(kept), 1), b, dtype=F), kept, np.full((len(kept), 1), c, dtype=F)], 1))
        if rows:
            rows = np.vstack(rows)                                               # class-major list of the kept rows
            best = rows[rank_desc_later_first(rows[:, 5])[:top_n]]
            det[b, :len(best)] = best
            counts[b] = len(best)
    return det, counts


# ------------------------------------------------------------------------------------------ box-prediction edge inputs ----------
PREDICT_CFG = {"bbox_normalize_stds": [0.1, 0.1, 0.2, 0.2], "bbox_normalize_means": [0, 0, 0, 0], "nms_iou_thresh": 0.5}


def _predict_inputs(B, P, C, counts, rois_of, score_of, info, seed, shift=1.0):
    """rois / prob / loc with NaN in every row >= counts[b]; loc: dx, dy uniform in [-shift, shift], size deltas 0 (exp(0) = 1 in
    every libm; 0 * std + 0 = 0)"""
    rs = np.random.RandomState(seed)
    rois = np.full((B * P, 5), np.nan, dtype=F)
    prob = np.full((B * P, C), np.nan, dtype=F)
    loc = np.full((B * P, 4 * C), np.nan, dtype=F)
    for b in range(B):
        m = counts[b]
        rois[b * P:b * P + m, 0] = b
        rois[b * P:b * P + m, 1:] = rois_of(rs, b, m)
        prob[b * P:b * P + m] = score_of(rs, b, m)
        d = rs.uniform(-shift, shift, (m, C, 4)).astype(F)
        d[:, :, 2:] = 0
        loc[b * P:b * P + m] = d.reshape(m, 4 * C)
    return dict(rois=rois, roi_counts=np.array(counts, dtype=np.int32), P=P, prob=prob, loc=loc, info=np.asarray(info, dtype=F))


def predict_case_a():
    """C = 81, P = 80, B = 2, score_thresh 0, disjoint 10-px RoIs on a 32-px pitch (the decode moves a box by at most 0.1 * 9 px, so
    they stay disjoint): every (row, class) is kept, 6400 keys per image sort in box_topn_kernel's workspace"""
    grid = lambda rs, b, m: disjoint_grid(m, cols=10, size=10, pitch=32, x0=8, y0=8)[:, :4]
    score = lambda rs, b, m: (np.floor(rs.uniform(0.05, 1.0, (m, 81)) * 512) / 512).astype(F)     # 9-bit scores: ties across classes
    return _predict_inputs(2, 80, 81, [80, 80], grid, score, [[400, 400, 1], [300, 340, 1]], 41)


def predict_case_b():
    """C = 2, P = 6150, B = 1, roi_counts 6150 on a disjoint grid: box_decode_sort_kernel's workspace branch (P > 6144); scores from 64
    levels: ties inside the class, so the low key bits decide"""
    grid = lambda rs, b, m: disjoint_grid(m, cols=82, size=10, pitch=16, x0=4, y0=4)[:, :4]
    score = lambda rs, b, m: (np.floor(rs.uniform(0.0, 1.0, (m, 2)) * 64 + 1) / 128).astype(F)
    return _predict_inputs(1, 6150, 2, [6150], grid, score, [[1300, 1400, 1]], 42, shift=0.5)


LEVELS = (0.25, 0.5, 0.625, 0.875)


def predict_case_c():
    """C = 9, P = 64, B = 3, roi_counts [64, 0, 17], a different image_info per image (image 2's clips), overlapping RoIs, scores
    from the 4 LEVELS: ties inside classes and across classes at the top_n cut; run with score_thresh = LEVELS[0] every score ON the
    threshold must be dropped"""
    def boxes(rs, b, m):
        x1, y1 = rs.randint(0, 200, m).astype(np.float64), rs.randint(0, 150, m).astype(np.float64)
        return np.stack([x1, y1, x1 + rs.randint(8, 90, m), y1 + rs.randint(8, 70, m)], 1)
    score = lambda rs, b, m: np.array(LEVELS, dtype=F)[rs.randint(0, 4, (m, 9))]
    return _predict_inputs(3, 64, 9, [64, 0, 17], boxes, score, [[240, 300, 1], [100, 100, 1], [120, 160, 2]], 43)


# --------------------------------------------------------------------------------------------------- box_ops edge inputs ----------
def threshold_anchor_case(gt_stride=5):
    """hand-built anchors / gts that sit ON every rule of anchor_label_kernel (thresholds neg 0.3, pos 0.7, min_gt_best 0.1):
      a0 [0,0,7,10]      IoU 70/100 = float32(0.7) with g0: NOT positive by the threshold, not negative -> -1
      a1 [0,0,10,10]     = g0: g0's best, positive by claim and by threshold
      a2 [0,0,3,10]      IoU 30/100 = float32(0.3) with g0: NOT negative -> -1
      a3 [100,0,110,9]   IoU 0.9 with g1 AND its duplicate g2, the best of both: claimed, best_gt = 2 (the LAST), argmax says 1
      a4 [300,300,310,310] IoU 1/100 with the tiny g3, g3's best but < 0.1: g3 claims nothing; a4 is negative
      a5 [500,500,510,510] touches nothing: best_iou 0, best_gt 0, negative
      a6 [100,0,105,10]  IoU 0.5 with g1: -1
    -> anchors float32 [7,4], gts float32 [4, gt_stride], expected labels"""
    anchors = np.array([[0, 0, 7, 10], [0, 0, 10, 10], [0, 0, 3, 10], [100, 0, 110, 9], [300, 300, 310, 310], [500, 500, 510, 510],
                        [100, 0, 105, 10]], dtype=F)
    gts = np.zeros((4, gt_stride), dtype=F)
    gts[:, :4] = [[0, 0, 10, 10], [100, 0, 110, 10], [100, 0, 110, 10], [300, 300, 301, 301]]
    gts[:, 4:] = 7
    return anchors, gts, np.array([-1, 1, -1, 1, 0, 0, -1], dtype=np.int8)


def random_anchor_case(KA, G, gt_stride, seed):
    """integer anchors (sides >= 4) and gts in a 160 x 160 field, dense enough that every label occurs; the first rows of the
    threshold case are planted when they fit.  Integer coordinates make many IoUs small rationals: ties between gts are common"""
    rs = np.random.RandomState(seed)
    x1, y1 = rs.randint(0, 120, KA), rs.randint(0, 120, KA)
    anchors = np.stack([x1, y1, x1 + rs.randint(4, 40, KA), y1 + rs.randint(4, 40, KA)], 1).astype(F)
    gx, gy = rs.randint(0, 120, G), rs.randint(0, 120, G)
    gts = np.zeros((G, gt_stride), dtype=F)
    gts[:, :4] = np.stack([gx, gy, gx + rs.randint(6, 40, G), gy + rs.randint(6, 40, G)], 1)
    gts[:, 4] = rs.randint(1, 9, G)
    if gt_stride > 5:
        gts[:, 5:] = np.nan                                      # padding columns: never read
    if G >= 2:
        gts[G - 1, :4] = gts[0, :4]                              # a duplicated gt: claims go to the last
    k = min(KA // 2, G)
    anchors[:k] = gts[:k, :4]                                    # some exact matches: positives by threshold
    for j in range(min(3, KA - k)):                              # half of a gt box: IoU about 0.5, neither positive nor negative
        g = gts[j % G, :4]
        anchors[k + j] = [g[0], g[1], g[0] + np.ceil((g[2] - g[0]) / 2), g[3]]
    for j in range(min(6, KA - k - 3)):                          # a gt box grown by a pixel: IoU >= 6/7, positive by threshold only
        anchors[k + 3 + j] = gts[j % G, :4] + np.array([0, 0, 1 + j % 2, (j // 2) % 2], dtype=F)
    return anchors, gts


def factor_KA(KA):
    """(A, fh, fw) with A*fh*fw = KA for the custom anchor arrays (anchor_finalize takes a grid shape)"""
    return {1: (1, 1, 1), 7: (7, 1, 1), 255: (15, 1, 17), 257: (1, 1, 257), 1023: (3, 11, 31), 1025: (5, 5, 41)}[KA]


def threshold_proposals(n_prop, seed, img_h=200, img_w=300):
    """proposal rows (b, x1, y1, x2, y2, score) [n_prop, 6] and gts [3, 5] for thresholds pos 0.7 / neg_hi 0.5 / neg_lo 0.1: the
    first rows sit ON each threshold against g0 = [0,0,10,10] (IoU 0.7: neither; 0.5: neither; 0.1: background), then boxes wholly
    outside the image (clipped to zero area: IoU 0 < neg_lo: neither), then random boxes partly outside"""
    rs = np.random.RandomState(seed)
    gts = np.array([[0, 0, 10, 10, 3], [150, 60, 260, 170, 5], [40, 100, 120, 190, 1]], dtype=F)
    x1, y1 = rs.uniform(-40, img_w + 20, n_prop), rs.uniform(-40, img_h + 20, n_prop)
    p = np.stack([np.zeros(n_prop), x1, y1, x1 + rs.uniform(4, 150, n_prop), y1 + rs.uniform(4, 120, n_prop),
                  np.sort(rs.uniform(0, 1, n_prop))[::-1]], 1).astype(F)
    planted = np.array([[0, 0, 1, 10], [0, 0, 7, 10], [0, 0, 5, 10], [-50, -60, -5, -8], [img_w + 5, 20, img_w + 90, 80],
                        [150, 60, 260, 168], [42, 100, 120, 190]], dtype=F)
    k = min(n_prop, len(planted))
    p[:k, 1:5] = planted[:k]
    return p, gts
