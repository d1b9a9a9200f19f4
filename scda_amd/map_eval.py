"""Cityscapes mAP on the device: a streaming evaluator over the Predictor's device-resident results (scda_amd/csrc/map_eval.hip).

It computes what the reference's utils/cal_mAP.py computes from the rows validate() writes (tools/faster_rcnn_train_val.py:826-858) --
per-class ap and max_recall, the mAP -- plus validate()'s RPN recall (bbox_helper.compute_recall), bit for bit; include/scda_ops.h
states the rules R1..R4, tests/voc_map_np.py restates them in numpy.  No text is written or parsed and nothing waits for the host before
summarize().

Where it differs from the file path, on purpose:
  * Equal scores inside one image: the keep_num best rows are chosen with ties in the GIVEN order, earlier first.  validate() uses
    argsort()[::-1], whose order among equal scores is numpy's; the two can keep or order tied rows differently.
  * A class without any row: ap = max_recall = 0 and rows = 0.  The reference raises ValueError there (np.max of an empty array).
  * Data-parallel validation: every rank fills an evaluator over its shard (add(..., image_ids=...)) and one collective merge()
    leaves every rank holding all rows (eval_base.StreamingEvaluator.merge, rules M1..M4 of include/scda_ops.h), bit-equal to what
    the reference computes from `cat results.txt.rank*`: the ranks in merge_order(world) -- the order of the decimal rank STRINGS --,
    inside a rank the images as added.  An image a DistributedSampler repeats as padding is not removed, as in the reference: the
    rows of every later copy stay and are false positives.  NOT covered: a repeated image whose copies carry different rows
    (summarize() raises ValueError).  With sum_gt=None a repeated image's ground truths count once per copy, because gt_num is
    summed over the ranks; the reference always divides by the meta file's counts, which is sum_gt=gt['num'].  The debug arrays are
    not merged.

    gt = evaluate.meta_ground_truth(val_meta_file, num_classes)
    ev = MapEvaluator(num_classes=9, max_images=500, max_dets_per_image=100, max_gts_per_image=128, device=dev, sum_gt=gt['num'])
    res = evaluate.map_stats(loader, predictor, ev, gt)       # {'ap', 'max_recall', 'mAP', 'mean_max_recall', 'rows', 'sum_gt', 'rpn_*'}
    res = evaluate.map_stats(loader, predictor, ev, gt, distributed=True)     # every rank: its shard, then the merged result"""
import numpy as np
import torch

from scda_amd import native as N
from scda_amd.eval_base import StreamingEvaluator, merge_order  # noqa: F401  (merge_order(world): the rank order of a merge)

MAX_PER_IMAGE = 1024
MAX_CLASSES = 256


class MapEvaluator(StreamingEvaluator):
    """Fixed-capacity streaming cal_mAP.  add() stores each image's rows (int32 box, score, class, kept flag, rank, true-positive flag)
    on the device; accumulate() sorts and scans all rows collected so far; summarize() brings 2 * num_classes doubles and the integer
    counters to the host.

    num_classes C <= 256 (classes 1..C-1), max_dets_per_image = the Predictor's top_n (<= 1024), max_gts_per_image = the capacity of the
    ground-truth tensors (<= 1024), keep_num <= max_dets_per_image (validate() keeps 100).  sum_gt: the meta file's per-class counts
    (meta_ground_truth(...)['num']), which count images that are never added too, as the reference does; None: the counts over the
    images added.  debug=True keeps .debug_match int32 [max_images, D] (the claimed ground truth's row of a true positive, else -1) and
    .debug_claimed int32 [max_images, G]; the true-positive flags .tp are always kept.  absorb() / merge() (eval_base) take the rows
    of sharded evaluators; they need add(..., image_ids=...)."""

    MERGE_ROWS = (('image_ids', 'minus_one'), ('box', 'zero'), ('score', 'zero'), ('cls', 'zero'), ('rank', 'slot'), ('kept', 'zero'),
                  ('tp', 'zero'))
    MERGE_COUNTERS = ('gt_num', 'rpn')

    def __init__(self, num_classes, max_images=500, max_dets_per_image=100, max_gts_per_image=128, device=None, iou_thr=0.5, keep_num=100,
                 sum_gt=None, debug=False):
        self.C, self.I = int(num_classes), int(max_images)
        self.D, self.G = int(max_dets_per_image), int(max_gts_per_image)
        self.iou_thr, self.keep_num = float(iou_thr), int(keep_num)
        if not (2 <= self.C <= MAX_CLASSES and self.I >= 1 and 1 <= self.D <= MAX_PER_IMAGE and 1 <= self.G <= MAX_PER_IMAGE):
            raise ValueError("MapEvaluator: 2 <= num_classes <= 256, max_images >= 1, 1 <= max_dets / max_gts per image <= 1024")
        if not 1 <= self.keep_num <= self.D:
            raise ValueError("MapEvaluator: 1 <= keep_num <= max_dets_per_image (%d), got %d" % (self.D, self.keep_num))
        self._init_stream(device)
        dev = self.device
        I, D, C = self.I, self.D, self.C
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=dev)        # noqa: E731
        self.d_sum_gt = None
        if sum_gt is not None:
            s = np.asarray(sum_gt)
            if s.shape != (C,) or np.any(s != np.floor(s)) or np.any(s < 0):
                raise ValueError("MapEvaluator: sum_gt must hold num_classes non-negative counts")
            self._sum_gt_host = s.astype(np.int32)
            self.d_sum_gt = N.upload(self._sum_gt_host, dev)
        # the rows
        self.image_ids = torch.full((I,), -1, dtype=torch.int32, device=dev)
        self._ids_missing = False
        self.box = z(I, D, 4, dtype=torch.int32)
        self.score = z(I, D, dtype=torch.float32)
        self.cls, self.rank, self.kept, self.tp = (z(I, D, dtype=torch.int32) for _ in range(4))
        self.debug_match = torch.full((I, D), -1, dtype=torch.int32, device=dev) if debug else None
        self.debug_claimed = z(I, self.G, dtype=torch.int32) if debug else None
        # the results: ap and max_recall; rows, the ground truths counted over the images added, the two recall counters
        self._f64 = z(2, C, dtype=torch.float64)
        self._i32 = z(2 * C + 2, dtype=torch.int32)
        self.rows, self.gt_num, self.rpn = self._i32[:C], self._i32[C:2 * C], self._i32[2 * C:]
        self.ws = torch.empty(max(N.map_accumulate_workspace_bytes(I, D), 16), dtype=torch.uint8, device=dev)

    def reset(self):
        self._i32.zero_()
        self._ids_missing = False
        self._reset_stream()

    def _merge_signature(self):
        return (self.C, self.I, self.D, self.G, self.iou_thr, self.keep_num,
                None if self.d_sum_gt is None else tuple(self._sum_gt_host.tolist()))

    def _check_mergeable(self):
        if self._ids_missing:
            raise ValueError("MapEvaluator: merging needs every image added with image_ids (-1: no identity)")

    def _apply_duplicates(self, first, n):
        N.map_merge_duplicates(first, n, self.box, self.score, self.cls, self.rank, self.kept, self.tp, self.merge_flags)

    @torch.no_grad()
    def add(self, detections, detection_counts, image_info, gt_boxes, gt_counts, proposals=None, proposal_counts=None, recall_gts=None,
            recall_gt_counts=None, scale_column=-1, image_ids=None):
        """One batch of B images.  detections float32 [B, top_n, 7] and detection_counts int32 [B] (the Predictor's), image_info float32
        [B, >= 2] = (h, w, ..., resize scale at scale_column), gt_boxes int32 [B, Gcap, 5] = (x1, y1, x2, y2, label) in the ORIGINAL image's
        coordinates as the meta file has them, gt_counts int32 [B] -- device tensors of exactly these types are used as they are (anything
        else is converted, which allocates).  The RPN recall part is optional: proposals float32 [B, P, >= 5] and proposal_counts int32
        [B] (the Predictor's), recall_gts float32 [B, Gr, >= 4] (validate()'s item[2], network-input coordinates) and recall_gt_counts
        int32 [B] (default: all Gr rows, padding included, as the reference counts them).  Capacity violations raise before anything is
        launched; the counts themselves live on the device and are clamped there.  image_ids int32 [B] (default: none; absorb() and
        merge() need them): what makes two images of different shards the same image, e.g. the position in the meta file; -1 = no
        identity, never a duplicate."""
        if not hasattr(detections, 'shape') or len(detections.shape) != 3 or detections.shape[1] != self.D or detections.shape[2] != 7:
            raise ValueError("MapEvaluator.add: detections must be [B, %d, 7] (max_dets_per_image = %d)" % (self.D, self.D))
        B = int(detections.shape[0])
        s0, s1 = self._slots(B)
        if len(gt_boxes.shape) != 3 or tuple(gt_boxes.shape[1:]) != (self.G, 5):
            raise ValueError("MapEvaluator.add: gt_boxes must be [B, %d, 5] (max_gts_per_image = %d)" % (self.G, self.G))
        if len(image_info.shape) != 2 or image_info.shape[0] != B or image_info.shape[1] < 2 or \
                not -image_info.shape[1] <= scale_column < image_info.shape[1]:
            raise ValueError("MapEvaluator.add: image_info must be [B, >= 2] and hold scale_column")
        recall = proposals is not None
        if recall:
            if proposal_counts is None or recall_gts is None:
                raise ValueError("MapEvaluator.add: the recall part needs proposals, proposal_counts and recall_gts")
            if len(proposals.shape) != 3 or proposals.shape[0] != B or proposals.shape[2] < 5 or len(recall_gts.shape) != 3 or \
                    recall_gts.shape[0] != B or recall_gts.shape[1] < 1 or recall_gts.shape[2] < 4:
                raise ValueError("MapEvaluator.add: proposals [B, P, >= 5] and recall_gts [B, Gr >= 1, >= 4]")
        det = self._dev(detections, "detections", torch.float32, (B, self.D, 7))
        dc = self._dev(detection_counts, "detection_counts", torch.int32, (B,))
        info = self._dev(image_info, "image_info", torch.float32, None)
        gb = self._dev(gt_boxes, "gt_boxes", torch.int32, (B, self.G, 5))
        gc = self._dev(gt_counts, "gt_counts", torch.int32, (B,))
        if recall:
            pr = self._dev(proposals, "proposals", torch.float32, None)
            pc = self._dev(proposal_counts, "proposal_counts", torch.int32, (B,))
            rg = self._dev(recall_gts, "recall_gts", torch.float32, None)
            if recall_gt_counts is None:
                recall_gt_counts = np.full(B, rg.shape[1], np.int32)
            rc = self._dev(recall_gt_counts, "recall_gt_counts", torch.int32, (B,))
        if image_ids is None:
            self._ids_missing = True
            self.image_ids[s0:s1].fill_(-1)
        else:
            self.image_ids[s0:s1].copy_(self._dev(image_ids, "image_ids", torch.int32, (B,)))
        dbg_m = None if self.debug_match is None else self.debug_match[s0:s1]
        dbg_c = None if self.debug_claimed is None else self.debug_claimed[s0:s1]
        N.map_rows(det, dc, info, scale_column, self.C, self.keep_num, self.box[s0:s1], self.score[s0:s1], self.cls[s0:s1],
                   self.rank[s0:s1], self.kept[s0:s1], self.tp[s0:s1], dbg_match=dbg_m, dbg_claimed=dbg_c, G=self.G)
        N.map_match(self.box[s0:s1], self.cls[s0:s1], self.rank[s0:s1], self.kept[s0:s1], gb, gc, self.C, self.iou_thr, self.tp[s0:s1],
                    self.gt_num, dbg_match=dbg_m, dbg_claimed=dbg_c)
        if recall:
            N.map_recall(pr, pc, rg, rc, self.rpn)
        self.n_images = s1

    @torch.no_grad()
    def accumulate(self):
        """-> {'ap' [C], 'max_recall' [C] float64, 'rows' [C] int32}: device tensors of the evaluator (overwritten by the next call),
        cal_mAP's arrays over every image added so far"""
        self._require_images()
        N.map_accumulate(self.n_images, self.score, self.cls, self.rank, self.kept, self.tp,
                         self.gt_num if self.d_sum_gt is None else self.d_sum_gt, self.ws, self._f64[0], self._f64[1], self.rows)
        self._accumulated = self.n_images
        return {'ap': self._f64[0], 'max_recall': self._f64[1], 'rows': self.rows}

    @torch.no_grad()
    def summarize(self):
        """-> {'ap', 'max_recall' float64 [C], 'mAP' = np.mean(ap[1:]), 'mean_max_recall', 'rows' [C], 'sum_gt' [C], 'rpn_recalled',
        'rpn_gts', 'rpn_recall' (nan without recall rows)}; the one host wait.  The means are numpy's over the doubles that crossed."""
        self._ensure_accumulated()
        f = self._f64.cpu().numpy()
        i = self._i32.cpu().numpy()
        self._check_merge_flags()
        C = self.C
        rc, ng = int(i[2 * C]), int(i[2 * C + 1])
        return {'ap': f[0].copy(), 'max_recall': f[1].copy(), 'mAP': np.mean(f[0][1:]), 'mean_max_recall': np.mean(f[1][1:]),
                'rows': i[:C].copy(), 'sum_gt': (i[C:2 * C] if self.d_sum_gt is None else self.d_sum_gt.cpu().numpy()).copy(),
                'rpn_recalled': rc, 'rpn_gts': ng, 'rpn_recall': rc / ng if ng else float('nan')}
