"""COCO AP on the device: a streaming evaluator over the Predictor's device-resident results (scda_amd/csrc/coco_eval.hip).

It computes what the reference's datasets/pycocotools/cocoeval.py computes -- COCOeval.evaluate(), accumulate(), summarize() -- for
iouType 'bbox' and 'segm' with useCats = 1 and the default detection parameters (10 IoU thresholds np.linspace(.5, .95, 10), 101 recall
thresholds, maxDets [1, 10, 100], the four area ranges), bit for bit for precision / recall / scores; include/scda_ops.h states the
rules, tests/coco_eval_np.py restates them in numpy.  The parameters are numpy values uploaded at construction, never kernel constants.

NOT covered: keypoints / OKS, useCats = 0 (proposal AR), the text / JSON round trip, annotation loading: ground truth arrives as device tensors
(scda_amd.coco_gt.GroundTruth builds them, masks included, from annotation dicts).  Detections and ground truth must be in the SAME coordinates -- dividing the
network-input detections by resize_scale (or scaling the ground truth) stays with the caller.  Image ids must be distinct.

Data-parallel validation: every rank fills an evaluator over its shard and one collective merge() leaves every rank holding all rows
and the summed npig / seen (eval_base.StreamingEvaluator.merge, rules M1..M3 of include/scda_ops.h); accumulate() orders the rows by
(image id, slot), so the order of the ranks has no effect.  The shards must be UNPADDED, e.g. Subset(ds, range(rank, n, world)): the
reference would evaluate an image a DistributedSampler repeats once more with both copies' detections cut at maxDets, which the stored
rows cannot reproduce (the ground truth is not kept) -- a repeated image id after the merge makes summarize() raise ValueError.  Only
the rows accumulate() reads are merged (not xywh, area or the debug array).

    ev = CocoEvaluator(num_categories=80, iou_type='bbox', max_images=5000, max_dets_per_image=100, max_gts_per_image=64, device=dev)
    for images, info, ids, gt in loader:                      # nothing below waits for the host
        out = predictor(images, info)
        ev.add(ids, out[2], out[3], gt.boxes, gt.areas, gt.iscrowd, gt.categories, gt.counts)
    stats = ev.summarize()                                    # 12 doubles cross to the host"""
import numpy as np
import torch

from scda_amd import native as N
from scda_amd.eval_base import StreamingEvaluator, merge_order  # noqa: F401

MAX_PER_IMAGE = 1024


def default_params():
    """Params.setDetParams (cocoeval.py:503-512), computed by numpy as the reference computes them"""
    return {'iou_thrs': np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            'rec_thrs': np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            'max_dets': [1, 10, 100],
            'area_rng': np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)}


def stat_specs(iou_thrs, max_dets):
    """_summarizeDets' 12 selections as (ap, t, a, m); t = -1: every threshold, -2: the list does not hold the value (np.where finds
    nothing and the reference reports -1); area ranges in the order all, small, medium, large.  max_dets is the sorted list.  The
    selection is the reference's: stats 1..5 and 8..11 take maxDets[2], stats 6 and 7 maxDets[0] and maxDets[1], and stat 0 is
    _summarize(1), whose default maxDets = 100 selects the entry EQUAL to 100 -- without one nothing is selected and the stat is -1
    (t = -2).  With fewer than three entries the reference cannot answer (IndexError on maxDets[2] / maxDets[1]): those selections then
    fall back to the last entry, as they always did here; stat 0 follows the reference there too."""
    def at(v):
        w = np.where(v == np.asarray(iou_thrs))[0]
        return int(w[0]) if len(w) else -2
    max_dets = [int(m) for m in max_dets]
    last = len(max_dets) - 1
    m0, m1, m2 = 0, min(1, last), min(2, last)
    t100, m100 = (-1, max_dets.index(100)) if 100 in max_dets else (-2, 0)
    return np.array([(1, t100, 0, m100), (1, at(.5), 0, m2), (1, at(.75), 0, m2), (1, -1, 1, m2), (1, -1, 2, m2), (1, -1, 3, m2),
                     (0, -1, 0, m0), (0, -1, 0, m1), (0, -1, 0, m2), (0, -1, 1, m2), (0, -1, 2, m2), (0, -1, 3, m2)], dtype=np.int32)


class CocoEvaluator(StreamingEvaluator):
    """Fixed-capacity streaming COCOeval.  add() stores each image's rows (score, category, rank and the matched / ignored masks of every
    detection slot) on the device; accumulate() sorts and scans all rows collected so far; summarize() returns the 12 stats.

    num_categories K <= 255 (category indices 1..K), max_dets_per_image = the Predictor's top_n (<= 1024), max_gts_per_image = the
    Gcap of the ground-truth tensors (<= 1024).  params: overrides of default_params() (e.g. scaled area ranges); the limits are 16
    thresholds, 8 area ranges (the summary uses the first four as all / small / medium / large), 4 maxDets, 128 recall thresholds.
    debug=True keeps the matched GT row of every (detection, area range, threshold) in .debug_match [max_images, D, A, T]."""

    MERGE_ROWS = (('image_ids', 'minus_one'), ('score', 'zero'), ('cat', 'zero'), ('rank', 'zero'), ('bits', 'zero'))
    MERGE_COUNTERS = ('npig', 'seen')
    MERGE_RAISES_ON_DUPLICATE = True

    def __init__(self, num_categories, iou_type='bbox', max_images=5000, max_dets_per_image=100, max_gts_per_image=64, device=None,
                 params=None, debug=False):
        if iou_type not in ('bbox', 'segm'):
            raise ValueError("CocoEvaluator: iou_type must be 'bbox' or 'segm' (keypoints are not covered)")
        p = dict(default_params(), **(params or {}))
        self.iou_type = iou_type
        self.K, self.I = int(num_categories), int(max_images)
        self.D, self.G = int(max_dets_per_image), int(max_gts_per_image)
        self.iou_thrs = np.asarray(p['iou_thrs'], dtype=np.float64)
        self.rec_thrs = np.asarray(p['rec_thrs'], dtype=np.float64)
        self.max_dets = sorted(int(m) for m in p['max_dets'])
        self.area_rng = np.asarray(p['area_rng'], dtype=np.float64).reshape(-1, 2)
        self.T, self.R, self.A, self.M = len(self.iou_thrs), len(self.rec_thrs), len(self.area_rng), len(self.max_dets)
        if not (1 <= self.K <= 255 and self.I >= 1 and 1 <= self.D <= MAX_PER_IMAGE and 1 <= self.G <= MAX_PER_IMAGE):
            raise ValueError("CocoEvaluator: 1 <= num_categories <= 255, max_images >= 1, 1 <= max_dets / max_gts per image <= 1024")
        if not (1 <= self.T <= 16 and 4 <= self.A <= 8 and 1 <= self.M <= 4 and 1 <= self.R <= 128):
            raise ValueError("CocoEvaluator: at most 16 IoU thresholds, 4..8 area ranges, 4 maxDets, 128 recall thresholds")
        self._init_stream(device)
        dev = self.device
        I, D, K, A, T = self.I, self.D, self.K, self.A, self.T
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=dev)        # noqa: E731
        self.d_iou_thrs, self.d_rec_thrs = N.upload(self.iou_thrs, dev), N.upload(self.rec_thrs, dev)
        self.d_area_rng = N.upload(self.area_rng, dev)
        self.d_max_dets = N.upload(np.asarray(self.max_dets, dtype=np.int32), dev)
        self.d_specs = N.upload(stat_specs(self.iou_thrs, self.max_dets), dev)
        # the rows
        self.image_ids = z(I, dtype=torch.int32)
        self.xywh, self.area = z(I, D, 4, dtype=torch.float64), z(I, D, dtype=torch.float64)
        self.score, self.cat, self.rank = z(I, D, dtype=torch.float32), z(I, D, dtype=torch.int32), z(I, D, dtype=torch.int32)
        self.bits = z(I, D, A, dtype=torch.int32)
        self.npig, self.seen = z(K, A, dtype=torch.int32), z(K, dtype=torch.int32)
        self.debug_match = torch.full((I, D, A, T), -1, dtype=torch.int32, device=dev) if debug else None
        # the results
        self.precision = z(T, self.R, K, A, self.M, dtype=torch.float64)
        self.scores = z(T, self.R, K, A, self.M, dtype=torch.float64)
        self.recall = z(T, K, A, self.M, dtype=torch.float64)
        self.stats = z(12, dtype=torch.float64)
        self.ws = torch.empty(max(N.coco_accumulate_workspace_bytes(I, D, K, A), 16), dtype=torch.uint8, device=dev)
        self._iou = None                        # [B, G, D] of the largest batch seen
        self._miou = None                       # 'segm': scda_mask_iou_hip's workspace and raw intersections

    def _merge_signature(self):
        return (self.iou_type, self.K, self.I, self.D, self.G, self.iou_thrs.tobytes(), self.rec_thrs.tobytes(), tuple(self.max_dets),
                self.area_rng.tobytes())

    def reset(self):
        self.npig.zero_(); self.seen.zero_()
        if self.debug_match is not None:
            self.debug_match.fill_(-1)
        self._reset_stream()

    @torch.no_grad()
    def add(self, image_ids, detections, detection_counts, gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts,
            mask_bits=None, det_areas=None, gt_mask_bits=None, sizes=None):
        """One batch of B images.  image_ids int32 [B]; detections float32 [B, top_n, 7] and detection_counts int32 [B] (the Predictor's);
        gt_boxes float64 [B, Gcap, 4] (x, y, w, h), gt_areas float64 [B, Gcap], gt_iscrowd uint8 [B, Gcap], gt_categories int32 [B, Gcap]
        (1..K), gt_counts int32 [B] -- device tensors of exactly these types are used as they are (anything else is converted, which
        allocates).  'segm' also takes mask_bits int32 [B, top_n, H, Wd] and det_areas int32 [B, top_n] (the Predictor's mask_bits and
        rle['area']), gt_mask_bits int32 [B, Gcap, H, Wd] (infer.pack_masks of the ground truth, empty planes as padding) and sizes: one
        (h, w) or B of them on the HOST -- the image inside the planes (default: the whole plane).  Capacity violations raise before
        anything is launched; the counts themselves live on the device and are clamped there."""
        B = int(detections.shape[0])
        if len(detections.shape) != 3 or detections.shape[1] != self.D or detections.shape[2] != 7:
            raise ValueError("CocoEvaluator.add: detections must be [B, %d, 7] (max_dets_per_image = %d)" % (self.D, self.D))
        s0, s1 = self._slots(B)
        if tuple(gt_boxes.shape[1:]) != (self.G, 4):
            raise ValueError("CocoEvaluator.add: gt_boxes must be [B, %d, 4] (max_gts_per_image = %d)" % (self.G, self.G))
        det = self._dev(detections, "detections", torch.float32, (B, self.D, 7))
        dc = self._dev(detection_counts, "detection_counts", torch.int32, (B,))
        ids = self._dev(image_ids, "image_ids", torch.int32, (B,))
        gb = self._dev(gt_boxes, "gt_boxes", torch.float64, (B, self.G, 4))
        ga = self._dev(gt_areas, "gt_areas", torch.float64, (B, self.G))
        gi = self._dev(gt_iscrowd, "gt_iscrowd", torch.uint8, (B, self.G))
        gk = self._dev(gt_categories, "gt_categories", torch.int32, (B, self.G))
        gc = self._dev(gt_counts, "gt_counts", torch.int32, (B,))
        segm = self.iou_type == 'segm'
        if segm:
            if mask_bits is None or det_areas is None or gt_mask_bits is None:
                raise ValueError("CocoEvaluator.add: 'segm' needs mask_bits, det_areas and gt_mask_bits")
            if mask_bits.dim() != 4 or tuple(mask_bits.shape[:2]) != (B, self.D) or gt_mask_bits.dim() != 4 or \
                    tuple(gt_mask_bits.shape) != (B, self.G) + tuple(mask_bits.shape[2:]):
                raise ValueError("CocoEvaluator.add: mask_bits [B, %d, H, Wd] and gt_mask_bits [B, %d, H, Wd]" % (self.D, self.G))
            H, Wd = int(mask_bits.shape[2]), int(mask_bits.shape[3])
            mask_bits = self._dev(mask_bits, "mask_bits", torch.int32, (B, self.D, H, Wd))
            gt_mask_bits = self._dev(gt_mask_bits, "gt_mask_bits", torch.int32, (B, self.G, H, Wd))
            det_areas = self._dev(det_areas, "det_areas", torch.int32, (B, self.D))
            sizes = [(H, 32 * Wd)] * B if sizes is None else [tuple(int(v) for v in s) for s in np.asarray(sizes).reshape(-1, 2)]
            sizes = sizes * B if len(sizes) == 1 else sizes
            if len(sizes) != B or any(not (1 <= h <= H and 1 <= w <= 32 * Wd) for h, w in sizes):
                raise ValueError("CocoEvaluator.add: sizes must be one or B (h, w) inside the %d x %d planes" % (H, 32 * Wd))
        if self._iou is None or self._iou.shape[0] < B:
            self._iou = torch.zeros(B, self.G, self.D, dtype=torch.float64, device=self.device)       # (first batch of this size only)
        self.image_ids[s0:s1].copy_(ids)
        N.coco_det_rows(det, dc, self.K, self.xywh[s0:s1], self.area[s0:s1], self.score[s0:s1], self.cat[s0:s1],
                        mask_area=det_areas if segm else None)
        iou = self._iou[:B]
        if segm:
            key = (H, Wd)
            if self._miou is None or self._miou[0] != key:
                need = N.mask_iou_workspace_bytes(self.D, self.G, H, Wd)
                if need == 0:
                    raise ValueError("CocoEvaluator.add: mask planes out of scda_mask_iou_hip's range")
                self._miou = (key, torch.empty(need, dtype=torch.uint8, device=self.device),
                              torch.empty(self.G, self.D, dtype=torch.int32, device=self.device))
            for b in range(B):                  # rleIou of every (GT slot, detection slot); empty padding planes give 0
                N.mask_iou(mask_bits[b], gt_mask_bits[b], sizes[b], iscrowd=gi[b], ws=self._miou[1], out=(iou[b], self._miou[2]))
        else:
            N.coco_box_iou(self.xywh[s0:s1], dc, gb, gc, gi, out=iou)
        N.coco_match(iou, dc, self.cat[s0:s1], self.score[s0:s1], self.area[s0:s1], gc, gk, ga, gi, self.K, self.d_iou_thrs,
                     self.d_area_rng, self.max_dets[-1], self.rank[s0:s1], self.bits[s0:s1], self.npig, self.seen,
                     dbg_match=None if self.debug_match is None else self.debug_match[s0:s1])
        self.n_images = s1

    @torch.no_grad()
    def accumulate(self):
        """-> {'precision' [T, R, K, A, M], 'recall' [T, K, A, M], 'scores' [T, R, K, A, M]}: float64 device tensors of the evaluator
        (overwritten by the next call), COCOeval.eval's arrays over every image added so far"""
        self._require_images()
        N.coco_accumulate(self.image_ids, self.n_images, self.cat, self.rank, self.score, self.bits, self.npig, self.seen,
                          self.d_rec_thrs, self.d_max_dets, self.max_dets[-1], self.T, self.ws, self.precision, self.recall, self.scores)
        self._accumulated = self.n_images
        return {'precision': self.precision, 'recall': self.recall, 'scores': self.scores}

    @torch.no_grad()
    def summarize(self):
        """-> numpy float64 [12]: COCOeval.stats (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl); the one host wait"""
        self._ensure_accumulated()
        N.coco_summarize(self.precision, self.recall, (self.T, self.R, self.K, self.A, self.M), self.d_specs, self.stats)
        stats = self.stats.cpu().numpy()
        self._check_merge_flags()
        return stats
