"""What the soft-NMS tests compare with: synthetic head outputs for the box prediction and functions/predict_bbox.py restated as one
plain numpy composition (decode, clip, threshold, sort, soft_nms, top-n) around the host loop of cython_nms.soft_nms, which
tests/test_soft_nms.py pins bit for bit to the reference's compiled soft_nms on every fixture case."""
import numpy as np

from scda_amd.dropin.extensions._cython_bbox import cython_nms

SETTINGS = {1: {'method': 'linear', 'sigma': 0.5, 'Nt': 0.3, 'threshold': 0.001},
            2: {'method': 'gaussian', 'sigma': 0.5, 'Nt': 0.3, 'threshold': 0.001}}


def synth_head(B=2, P=64, C=4, counts=(64, 37), empty_class=2, H=200, W=312, seed=0):
    """-> rois [B*P,5] f32 (rows past an image's count: the degenerate RoI), counts i32 [B], prob [B*P,C] f32 (soft-max; class
    `empty_class` has probability 0 everywhere, below any positive threshold), loc [B*P,4C] f32, info [B,3] f32.  The RoIs stand in
    clusters of 8, so most of a class list overlaps something."""
    rs = np.random.RandomState(seed)
    rois = np.zeros((B * P, 5), dtype=np.float32)
    for b in range(B):
        k = (P + 7) // 8
        x1, y1 = rs.uniform(0, W - 100, k), rs.uniform(0, H - 80, k)
        base = np.stack([x1, y1, x1 + rs.uniform(20, 90, k), y1 + rs.uniform(16, 70, k)], 1)
        box = np.repeat(base, 8, 0)[:P] + rs.uniform(-6, 6, (P, 4))
        box[:, 0::2] = np.clip(box[:, 0::2], 0, W - 1); box[:, 1::2] = np.clip(box[:, 1::2], 0, H - 1)
        box[:, 2:] = np.maximum(box[:, 2:], box[:, :2])
        rois[b * P:(b + 1) * P, 0] = b
        rois[b * P:b * P + counts[b], 1:] = box[rs.permutation(P)][:counts[b]]
    logits = rs.randn(B * P, C) * 2
    e = np.exp(logits - logits.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32)
    prob[:, empty_class] = 0
    loc = (rs.randn(B * P, 4 * C) * 0.5).astype(np.float32)
    info = np.array([[H, W, 1.0]] * B, dtype=np.float32)
    return rois, np.array(counts, dtype=np.int32), prob, loc, info


def real_rows(counts, P):
    return np.concatenate([np.arange(b * P, b * P + int(c)) for b, c in enumerate(counts)])


def predict_rows(rois, prob, loc, info, cfg, soft):
    """rois [R,5] (real rows only), prob [R,C], loc [R,4C], info [B,>=2] -> float32 [m,7] = (b, x1, y1, x2, y2, score, class): per
    (class, image) decode in float64 (float32 centre form, float32 deltas * float64 stds + means), clip, scores > score_thresh,
    descending by score (equal scores: the later row first), rows cast to float32, soft_nms(*soft); per image the top_n by the
    rescored score (equal scores: the later row of the class-major list first)"""
    sigma, Nt, threshold, method = soft['sigma'], soft['Nt'], soft['threshold'], {'hard': 0, 'linear': 1, 'gaussian': 2}[soft['method']]
    stds, means = np.array(cfg['bbox_normalize_stds'], dtype=np.float64), np.array(cfg['bbox_normalize_means'], dtype=np.float64)
    C = prob.shape[1]
    n_img = int(rois[:, 0].max()) + 1
    x1, y1, x2, y2 = (rois[:, k] for k in range(1, 5))
    cx, cy, w, h = (x1 + x2) / np.float32(2), (y1 + y2) / np.float32(2), x2 - x1, y2 - y1          # float32
    rows = []
    for cls in range(1, C):
        d = loc[:, 4 * cls:4 * cls + 4].astype(np.float64) * stds + means
        ncx, ncy = d[:, 0] * w + cx, d[:, 1] * h + cy
        hw, hh = np.exp(d[:, 2]) * w / 2., np.exp(d[:, 3]) * h / 2.
        boxes = np.stack([ncx - hw, ncy - hh, ncx + hw, ncy + hh], 1)
        for b in range(n_img):
            idx = np.where(rois[:, 0] == b)[0]
            hi_x, hi_y = float(info[b, 1] - np.float32(1)), float(info[b, 0] - np.float32(1))
            bb = boxes[idx].copy()
            bb[:, 0::2] = np.minimum(np.maximum(bb[:, 0::2], 0.), hi_x)
            bb[:, 1::2] = np.minimum(np.maximum(bb[:, 1::2], 0.), hi_y)
            sc = prob[idx, cls]
            if cfg['score_thresh'] > 0:
                above = np.where(sc > np.float32(cfg['score_thresh']))[0]
                sc, bb = sc[above], bb[above]
            if sc.size == 0:
                continue
            order = np.argsort(sc, kind='stable')[::-1]
            cand = np.concatenate([bb[order], sc[order, None]], 1).astype(np.float32)
            kept, _ = cython_nms.soft_nms(cand, sigma=sigma, Nt=Nt, threshold=threshold, method=method)
            n = kept.shape[0]
            rows.append(np.concatenate([np.full((n, 1), b, np.float32), kept, np.full((n, 1), cls, np.float32)], 1))
    rows = np.concatenate(rows, 0)
    best = []
    for b in range(n_img):
        of_b = rows[rows[:, 0] == b]
        best.append(of_b[np.argsort(of_b[:, 5], kind='stable')[::-1][:cfg['top_n']]])
    return np.concatenate(best, 0).astype(np.float32)
