"""Detections from RCNN outputs at test time (the contract of the reference's functions/predict_bbox.py:13-66).

Pipeline per (class 1..C-1, image): decode the class's box deltas against the RoIs (de-normalised by the configured
stds/means), clip to the image, drop scores <= score_thresh, order by score, NMS on the device (or, with the optional cfg key
`soft_nms`, soft-NMS with its rescoring: native.soft_nms_setting describes the dict), tag with image and class; finally keep the
top_n detections of each image over all classes.  Row layout: (image, x1, y1, x2, y2, score, class).
Result order (class-major, image-minor, then the per-image top_n cut) is the reference's: ties in the final argsort resolve
the same way."""
import numpy as np
import torch

from scda_amd import native
from scda_amd.dropin import backend
from scda_amd.dropin.utils import bbox_helper


def _candidates_of(scores, boxes, image_hw, cfg, stable=False):
    """one (image, class) pair -> its boxes [k,5] clipped, thresholded and ordered by score (descending), or None.  stable: equal
    scores in the order the device path states (the later row first) instead of whatever numpy's default argsort leaves"""
    boxes[:, :4] = bbox_helper.clip_bbox(boxes[:, :4], image_hw)
    if cfg['score_thresh'] > 0:
        above = np.where(scores > cfg['score_thresh'])[0]
        scores, boxes = scores[above], boxes[above]
    if scores.size == 0:
        return None
    return boxes[scores.argsort(kind='stable' if stable else None)[::-1], :]


def compute_predicted_bboxes(rois, pred_cls, pred_loc, image_info, cfg):
    out_device = rois.device if torch.is_tensor(rois) else torch.device('cpu')
    rois, pred_cls, pred_loc, image_info = (backend.host_array(t) for t in (rois, pred_cls, pred_loc, image_info))
    n_rois, n_cls = pred_cls.shape[0:2]
    assert n_rois == rois.shape[0]
    n_img = int(max(rois[:, 0].astype(np.int32)) + 1)
    members = [np.where(rois[:, 0] == b)[0] for b in range(n_img)]
    stds, means = np.array(cfg['bbox_normalize_stds'])[None, :], np.array(cfg['bbox_normalize_means'])[None, :]

    # every (class, image) list first, then ONE batched NMS over all of them (one upload, a mask and a sweep launch with one
    # workgroup per list, one download) instead of (classes - 1) x images round trips
    # the optional `soft_nms` key; with it equal scores are ordered by the device path's stated rule in both sorts below (numpy's
    # default argsort leaves their order undefined, and soft-NMS, unlike the hard NMS, has no reference wiring whose order to keep),
    # so that this function and scda_amd.infer.Predictor give the same rows on the same head outputs, ties included
    soft = native.soft_nms_setting(cfg.get('soft_nms'))
    lists, tags = [], []
    for cls in range(1, n_cls):
        scores = pred_cls[:, cls].squeeze()
        deltas = pred_loc[:, 4 * cls:4 * cls + 4].squeeze()
        if cfg['bbox_normalize_stats_precomputed']:
            deltas = deltas * stds + means
        scored = np.hstack([bbox_helper.compute_loc_bboxes(rois[:, 1:5], deltas), scores[:, None]])
        for b, idx in enumerate(members):
            cand = _candidates_of(scores[idx], scored[idx], image_info[b], cfg, stable=soft is not None)
            if cand is not None:
                lists.append(cand)
                tags.append((b, cls))
    rows = []
    if soft is None:
        kept_lists = [cand[np.asarray(keep, dtype=np.int64)] for cand, keep in zip(lists, backend.nms_segments(lists, cfg['nms_iou_thresh']))]
    else:
        # cython_nms.soft_nms on the float32 rows (what it accepts, and what the device path holds at this
        # point) in place of the hard NMS; its returned rows carry the rescored scores, in selection order
        kept_lists = [kept for kept, _ in backend.soft_nms_segments([c.astype(np.float32) for c in lists], *soft)]
    for kept, (b, cls) in zip(kept_lists, tags):
        n = kept.shape[0]
        rows.append(np.hstack([np.full((n, 1), b), kept, np.full((n, 1), cls)]))
    rows = np.vstack(rows)
    if cfg['top_n'] > 0:
        best = []
        for b in range(n_img):
            of_b = rows[rows[:, 0] == b]
            best.append(of_b[of_b[:, -2].argsort(kind='stable' if soft is not None else None)[::-1][:cfg['top_n']]])
        rows = np.vstack(best)
    return torch.from_numpy(rows).float().to(out_device)
