"""COCO AP on the device: a streaming evaluator over the Predictor's device-resident results (scda_amd/csrc/coco_eval.hip).

It computes what the reference's datasets/pycocotools/cocoeval.py computes -- COCOeval.evaluate(), accumulate(), summarize() -- for
iouType 'bbox' and 'segm' with the default detection parameters (10 IoU thresholds np.linspace(.5, .95, 10), 101 recall thresholds,
maxDets [1, 10, 100], the four area ranges), bit for bit for precision / recall / scores; include/scda_ops.h states the rules,
tests/coco_eval_np.py restates them in numpy.  The parameters are numpy values uploaded at construction, never kernel constants.

Every test type of the reference's utils/coco_eval.py is covered:
  'bbox', 'segm', 'person_bbox'      CocoEvaluator(K, 'bbox' | 'segm')
  'proposal', 'person_proposal'      CocoEvaluator(K, 'bbox', use_cats=False, params={'max_dets': [1, 100, 1000]}): useCats = 0, fed
                                     the Predictor's proposals through add_proposals() or class rows through add()
  'keypoints'                        CocoEvaluator(K, 'keypoints', num_keypoints=17): computeOks, Params.setKpParams, _summarizeKps
                                     (10 stats); the keypoint detections come from infer.Predictor(keypoints=True) through
                                     evaluate.coco_stats, or from the caller as device tensors (tests/coco_kps_np.py restates the
                                     rules)

NOT covered: useCats = 0 for keypoints (the reference then evaluates
nothing), the text / JSON round trip, annotation loading: ground truth arrives as device tensors
(scda_amd.coco_gt.GroundTruth builds them, masks included, from annotation dicts).  Detections and ground truth must be in the SAME coordinates -- dividing the
network-input detections by resize_scale (or scaling the ground truth) stays with the caller.  Image ids must be distinct.

Data-parallel validation: every rank fills an evaluator over its shard and one collective merge() leaves every rank holding all rows
and the summed npig / seen (eval_base.StreamingEvaluator.merge, rules M1..M3 of include/scda_ops.h); accumulate() orders the rows by
(image id, slot), so the order of the ranks has no effect.  The shards must be UNPADDED, e.g. Subset(ds, range(rank, n, world)): the
reference would evaluate an image a DistributedSampler repeats once more with both copies' detections cut at maxDets, which the stored
rows cannot reproduce (the ground truth is not kept) -- a repeated image id after the merge makes summarize() raise ValueError.  Only
the rows accumulate() reads are merged (not xywh, area or the debug arrays).

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
MAX_KEYPOINTS = 32


def default_params(iou_type='bbox'):
    """Params.setDetParams (cocoeval.py:503-512) or, for 'keypoints', Params.setKpParams (:514-523) with computeOks' sigmas (:206),
    computed by numpy as the reference computes them"""
    p = {'iou_thrs': np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
         'rec_thrs': np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)}
    if iou_type == 'keypoints':
        p['max_dets'] = [20]
        p['area_rng'] = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
        p['sigmas'] = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
    else:
        p['max_dets'] = [1, 10, 100]
        p['area_rng'] = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
    return p


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


def kps_stat_specs(iou_thrs, max_dets):
    """_summarizeKps' 10 selections (cocoeval.py:474-486) as (ap, t, a, m), t as in stat_specs: AP, AP50, AP75, APmedium, APlarge and
    the same five for AR; area ranges in the order all, medium, large; every one at the maxDets entry EQUAL to 20 -- a list without a
    20 selects nothing and every stat is -1 (t = -2)."""
    def at(v):
        w = np.where(v == np.asarray(iou_thrs))[0]
        return int(w[0]) if len(w) else -2
    max_dets = [int(m) for m in max_dets]
    have = 20 in max_dets
    m = max_dets.index(20) if have else 0
    sel = lambda t: t if have else -2                                         # noqa: E731
    five = [(sel(-1), 0), (sel(at(.5)), 0), (sel(at(.75)), 0), (sel(-1), 1), (sel(-1), 2)]
    return np.array([(ap, t, a, m) for ap in (1, 0) for t, a in five], dtype=np.int32)


class CocoEvaluator(StreamingEvaluator):
    """Fixed-capacity streaming COCOeval.  add() stores each image's rows (score, category, rank and the matched / ignored masks of every
    detection slot) on the device; accumulate() sorts and scans all rows collected so far; summarize() returns the stats: 12 for
    'bbox' / 'segm', 10 for 'keypoints'.

    num_categories K <= 255 (category indices 1..K), max_dets_per_image = the Predictor's top_n (<= 1024), max_gts_per_image = the
    Gcap of the ground-truth tensors (<= 1024).  params: overrides of default_params(iou_type) (e.g. scaled area ranges); the limits are
    16 thresholds, 8 area ranges (at least four -- the summary uses the first four as all / small / medium / large --, for keypoints at
    least three: all / medium / large), 4 maxDets, 128 recall thresholds; for keypoints 'sigmas' float64 [Kp], Kp <= 32 (only the
    default 17 are pinned to the reference).
    num_keypoints: Kp of add()'s keypoint tensors, a capacity like max_dets_per_image with no default: 'keypoints' needs it (the bare
    CocoEvaluator(K, 'keypoints') raises, as it did before keypoints were covered), it must equal len(sigmas), and no other iou_type
    takes it.
    use_cats=False: COCOeval's useCats = 0 (proposal AR).  num_categories still bounds the incoming class column (a slot whose class is
    outside 1..K takes no part), but the result arrays have K = 1: every image's rows are regrouped on the device into the reference's
    order -- category ascending, then the order given -- before the matching (scda_coco_regroup_hip).  Refused for keypoints: the
    reference's computeOks then finds no ground truth and evaluates nothing.
    debug=True keeps the matched GT row of every (detection, area range, threshold) in .debug_match [max_images, D, A, T]; with
    use_cats=False the rows it names are the REGROUPED ones and .perm_dets [max_images, D] / .perm_gts [max_images, G] hold the given
    slot / row standing at each regrouped place (-1 behind the live ones)."""

    MERGE_ROWS = (('image_ids', 'minus_one'), ('score', 'zero'), ('cat', 'zero'), ('rank', 'zero'), ('bits', 'zero'))
    MERGE_COUNTERS = ('npig', 'seen')
    MERGE_RAISES_ON_DUPLICATE = True

    def __init__(self, num_categories, iou_type='bbox', max_images=5000, max_dets_per_image=100, max_gts_per_image=64, device=None,
                 params=None, debug=False, use_cats=True, num_keypoints=None):
        if iou_type not in ('bbox', 'segm', 'keypoints'):
            raise ValueError("CocoEvaluator: iou_type must be 'bbox', 'segm' or 'keypoints'")
        self.kps = iou_type == 'keypoints'
        if self.kps != (num_keypoints is not None):
            # Kp is a capacity of add()'s tensors like max_dets_per_image, and it has no default: the bare call CocoEvaluator(K,
            # 'keypoints') raises as it always did, a keypoint evaluator is asked for by naming its Kp
            raise ValueError("CocoEvaluator: iou_type 'keypoints' needs num_keypoints (Kp of the keypoint tensors, = len(sigmas)), and "
                             "only 'keypoints' takes it")
        self.use_cats = bool(use_cats)
        if self.kps and not self.use_cats:
            raise ValueError("CocoEvaluator: use_cats=False is not covered for 'keypoints' (the reference evaluates nothing there)")
        p = dict(default_params(iou_type), **(params or {}))
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
        if not (1 <= self.T <= 16 and (3 if self.kps else 4) <= self.A <= 8 and 1 <= self.M <= 4 and 1 <= self.R <= 128):
            raise ValueError("CocoEvaluator: at most 16 IoU thresholds, 4..8 area ranges (3..8 for keypoints), 4 maxDets, 128 recall "
                             "thresholds")
        self.sigmas = np.asarray(p['sigmas'], dtype=np.float64).reshape(-1) if self.kps else None
        if self.kps and not (1 <= len(self.sigmas) <= MAX_KEYPOINTS and len(self.sigmas) == int(num_keypoints)):
            raise ValueError("CocoEvaluator: 1..%d keypoint sigmas, as many as num_keypoints (%s given, %d sigmas)"
                             % (MAX_KEYPOINTS, num_keypoints, len(self.sigmas)))
        self.Kp = len(self.sigmas) if self.kps else 0
        self.KE = self.K if self.use_cats else 1                              # the K of the result arrays
        self._init_stream(device)
        dev = self.device
        I, D, K, A, T = self.I, self.D, self.KE, self.A, self.T
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=dev)        # noqa: E731
        self.d_iou_thrs, self.d_rec_thrs = N.upload(self.iou_thrs, dev), N.upload(self.rec_thrs, dev)
        self.d_area_rng = N.upload(self.area_rng, dev)
        self.d_max_dets = N.upload(np.asarray(self.max_dets, dtype=np.int32), dev)
        specs = kps_stat_specs(self.iou_thrs, self.max_dets) if self.kps else stat_specs(self.iou_thrs, self.max_dets)
        self.d_specs = N.upload(specs, dev)
        self.d_vars = N.upload((self.sigmas * 2) ** 2, dev) if self.kps else None
        # the rows
        self.image_ids = z(I, dtype=torch.int32)
        self.xywh, self.area = z(I, D, 4, dtype=torch.float64), z(I, D, dtype=torch.float64)
        self.score, self.cat, self.rank = z(I, D, dtype=torch.float32), z(I, D, dtype=torch.int32), z(I, D, dtype=torch.int32)
        self.bits = z(I, D, A, dtype=torch.int32)
        self.npig, self.seen = z(K, A, dtype=torch.int32), z(K, dtype=torch.int32)
        self.debug_match = torch.full((I, D, A, T), -1, dtype=torch.int32, device=dev) if debug else None
        keep_perm = debug and not self.use_cats
        self.perm_dets = torch.full((I, D), -1, dtype=torch.int32, device=dev) if keep_perm else None
        self.perm_gts = torch.full((I, self.G), -1, dtype=torch.int32, device=dev) if keep_perm else None
        # the results
        self.precision = z(T, self.R, K, A, self.M, dtype=torch.float64)
        self.scores = z(T, self.R, K, A, self.M, dtype=torch.float64)
        self.recall = z(T, K, A, self.M, dtype=torch.float64)
        self.stats = z(len(specs), dtype=torch.float64)
        self.ws = torch.empty(max(N.coco_accumulate_workspace_bytes(I, D, K, A), 16), dtype=torch.uint8, device=dev)
        self._iou = None                        # [B, G, D] of the largest batch seen
        self._miou = None                       # 'segm': scda_mask_iou_hip's workspace and raw intersections
        self._gign = None                       # 'keypoints': the GTs' ignore flags [B, G] of the largest batch seen
        self._given = None                      # use_cats=False: the batch's rows and IoU block in the order given, and the regrouped GT rows

    def _merge_signature(self):
        return (self.iou_type, self.K, self.I, self.D, self.G, self.iou_thrs.tobytes(), self.rec_thrs.tobytes(), tuple(self.max_dets),
                self.area_rng.tobytes(), self.use_cats, None if self.sigmas is None else self.sigmas.tobytes())

    def reset(self):
        self.npig.zero_(); self.seen.zero_()
        if self.debug_match is not None:
            self.debug_match.fill_(-1)
        if self.perm_dets is not None:
            self.perm_dets.fill_(-1); self.perm_gts.fill_(-1)
        self._reset_stream()

    def _ground_truth(self, B, gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts):
        if tuple(gt_boxes.shape[1:]) != (self.G, 4):
            raise ValueError("CocoEvaluator.add: gt_boxes must be [B, %d, 4] (max_gts_per_image = %d)" % (self.G, self.G))
        return (self._dev(gt_boxes, "gt_boxes", torch.float64, (B, self.G, 4)), self._dev(gt_areas, "gt_areas", torch.float64, (B, self.G)),
                self._dev(gt_iscrowd, "gt_iscrowd", torch.uint8, (B, self.G)),
                self._dev(gt_categories, "gt_categories", torch.int32, (B, self.G)), self._dev(gt_counts, "gt_counts", torch.int32, (B,)))

    def _row_targets(self, B, s0, s1):
        """where the rows kernel writes: the stored rows, or with use_cats=False the batch's buffers in the order given"""
        if self._iou is None or self._iou.shape[0] < B:
            self._iou = torch.zeros(B, self.G, self.D, dtype=torch.float64, device=self.device)       # (first batch of this size only)
        if self.use_cats:
            return self.xywh[s0:s1], self.area[s0:s1], self.score[s0:s1], self.cat[s0:s1]
        if self._given is None or self._given['iou'].shape[0] < B:
            z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=self.device)    # noqa: E731
            D, G = self.D, self.G
            self._given = {'xywh': z(B, D, 4, dtype=torch.float64), 'area': z(B, D, dtype=torch.float64),
                           'score': z(B, D, dtype=torch.float32), 'cat': z(B, D, dtype=torch.int32),
                           'iou': z(B, G, D, dtype=torch.float64), 'gt_area': z(B, G, dtype=torch.float64),
                           'gt_iscrowd': z(B, G, dtype=torch.uint8), 'gt_cat': z(B, G, dtype=torch.int32),
                           'perm_dets': z(B, D, dtype=torch.int32), 'perm_gts': z(B, G, dtype=torch.int32)}
        g = self._given
        return g['xywh'][:B], g['area'][:B], g['score'][:B], g['cat'][:B]

    def _match(self, B, s0, s1, dc, ga, gi, gk, gc, gt_ignore=None):
        """the batch's IoU block (self._iou[:B], in the order given) through the regroup, if any, and the matching"""
        iou = self._iou[:B]
        if not self.use_cats:
            g = self._given
            pd, pg = (g['perm_dets'][:B], g['perm_gts'][:B]) if self.perm_dets is None else (self.perm_dets[s0:s1], self.perm_gts[s0:s1])
            N.coco_regroup(self.K, dc, g['xywh'][:B], g['area'][:B], g['score'][:B], g['cat'][:B], gc, gk, ga, gi, iou,
                           self.xywh[s0:s1], self.area[s0:s1], self.score[s0:s1], self.cat[s0:s1], g['gt_area'][:B], g['gt_iscrowd'][:B],
                           g['gt_cat'][:B], g['iou'][:B], pd, pg)
            iou, ga, gi, gk = g['iou'][:B], g['gt_area'][:B], g['gt_iscrowd'][:B], g['gt_cat'][:B]
        args = (self.KE, self.d_iou_thrs, self.d_area_rng, self.max_dets[-1], self.rank[s0:s1], self.bits[s0:s1], self.npig, self.seen)
        dbg = None if self.debug_match is None else self.debug_match[s0:s1]
        if self.kps:
            N.coco_match_ign(iou, dc, self.cat[s0:s1], self.score[s0:s1], self.area[s0:s1], gc, gk, ga, gi, gt_ignore, *args, dbg_match=dbg)
        else:
            N.coco_match(iou, dc, self.cat[s0:s1], self.score[s0:s1], self.area[s0:s1], gc, gk, ga, gi, *args, dbg_match=dbg)
        self.n_images = s1

    @torch.no_grad()
    def add(self, image_ids, detections, detection_counts, gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts,
            mask_bits=None, det_areas=None, gt_mask_bits=None, sizes=None, keypoints=None, gt_keypoints=None, gt_num_keypoints=None):
        """One batch of B images.  image_ids int32 [B]; detections float32 [B, top_n, 7] and detection_counts int32 [B] (the Predictor's);
        gt_boxes float64 [B, Gcap, 4] (x, y, w, h), gt_areas float64 [B, Gcap], gt_iscrowd uint8 [B, Gcap], gt_categories int32 [B, Gcap]
        (1..K), gt_counts int32 [B] -- device tensors of exactly these types are used as they are (anything else is converted, which
        allocates).  'segm' also takes mask_bits int32 [B, top_n, H, Wd] and det_areas int32 [B, top_n] (the Predictor's mask_bits and
        rle['area']), gt_mask_bits int32 [B, Gcap, H, Wd] (infer.pack_masks of the ground truth, empty planes as padding) and sizes: one
        (h, w) or B of them on the HOST -- the image inside the planes (default: the whole plane).
        'keypoints' also takes keypoints float32 [B, top_n, Kp, 3] (x, y, anything; each value is cast to double, as the reference's
        float32 results become Python floats), gt_keypoints float64 [B, Gcap, Kp, 3] (x, y, v) and gt_num_keypoints int32 [B, Gcap], the
        annotation's own field: it decides the GT's ignore flag while the OKS counts v > 0 itself, as in the reference.  detections then
        supply score and class only; the box and area of a detection are the extent of its Kp points.
        Capacity violations raise before anything is launched; the counts themselves live on the device and are clamped there."""
        B = int(detections.shape[0])
        if len(detections.shape) != 3 or detections.shape[1] != self.D or detections.shape[2] != 7:
            raise ValueError("CocoEvaluator.add: detections must be [B, %d, 7] (max_dets_per_image = %d)" % (self.D, self.D))
        s0, s1 = self._slots(B)
        gt = (gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts)
        if self.kps:
            if keypoints is None or gt_keypoints is None or gt_num_keypoints is None:
                raise ValueError("CocoEvaluator.add: 'keypoints' needs keypoints, gt_keypoints and gt_num_keypoints")
            if tuple(keypoints.shape) != (B, self.D, self.Kp, 3) or tuple(gt_keypoints.shape) != (B, self.G, self.Kp, 3):
                raise ValueError("CocoEvaluator.add: keypoints [B, %d, %d, 3] and gt_keypoints [B, %d, %d, 3] (Kp = len(sigmas))"
                                 % (self.D, self.Kp, self.G, self.Kp))
        gb, ga, gi, gk, gc = self._ground_truth(B, *gt)
        det = self._dev(detections, "detections", torch.float32, (B, self.D, 7))
        dc = self._dev(detection_counts, "detection_counts", torch.int32, (B,))
        ids = self._dev(image_ids, "image_ids", torch.int32, (B,))
        segm = self.iou_type == 'segm'
        if self.kps:
            kp = self._dev(keypoints, "keypoints", torch.float32, (B, self.D, self.Kp, 3))
            gkp = self._dev(gt_keypoints, "gt_keypoints", torch.float64, (B, self.G, self.Kp, 3))
            gnk = self._dev(gt_num_keypoints, "gt_num_keypoints", torch.int32, (B, self.G))
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
        xywh, area, score, cat = self._row_targets(B, s0, s1)
        self.image_ids[s0:s1].copy_(ids)
        if self.kps:
            N.coco_kp_rows(det, dc, kp, self.K, xywh, area, score, cat)
        else:
            N.coco_det_rows(det, dc, self.K, xywh, area, score, cat, mask_area=det_areas if segm else None)
        iou = self._iou[:B]
        gign = None
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
        elif self.kps:
            if self._gign is None or self._gign.shape[0] < B:
                self._gign = torch.zeros(B, self.G, dtype=torch.uint8, device=self.device)
            gign = self._gign[:B]
            N.coco_oks(kp, dc, gkp, gb, ga, gc, self.d_vars, out=iou, gt_iscrowd=gi, gt_num_keypoints=gnk, gt_ignore=gign)
        else:
            N.coco_box_iou(xywh, dc, gb, gc, gi, out=iou)
        self._match(B, s0, s1, dc, ga, gi, gk, gc, gt_ignore=gign)

    @torch.no_grad()
    def add_proposals(self, image_ids, proposals, proposal_counts, gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts,
                      xyxy_as_xywh=False):
        """One batch of B images scored by its RPN proposals (the reference's test types 'proposal' / 'person_proposal'): proposals
        float32 [B, P, 6] = (b, x1, y1, x2, y2, score) with P = max_dets_per_image and proposal_counts int32 [B] -- the Predictor's out[0],
        out[1] --, every proposal of category 1; the ground truth as in add().  The evaluator must be a 'bbox' one built with
        use_cats=False.
        xyxy_as_xywh=True reproduces a DEFECT of the reference bit for bit: for 'proposal' utils/coco_eval.py:33-36 hands
        [x1, y1, x2, y2] to COCO as if it were [x, y, w, h], so every box is too large by its own corner.  The default computes
        w = (double) x2 - (double) x1 like the detection rows."""
        if self.use_cats or self.iou_type != 'bbox':
            raise ValueError("CocoEvaluator.add_proposals: needs a 'bbox' evaluator built with use_cats=False")
        B = int(proposals.shape[0])
        if len(proposals.shape) != 3 or proposals.shape[1] != self.D or proposals.shape[2] != 6:
            raise ValueError("CocoEvaluator.add_proposals: proposals must be [B, %d, 6] (max_dets_per_image = %d)" % (self.D, self.D))
        s0, s1 = self._slots(B)
        gb, ga, gi, gk, gc = self._ground_truth(B, gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts)
        prop = self._dev(proposals, "proposals", torch.float32, (B, self.D, 6))
        pc = self._dev(proposal_counts, "proposal_counts", torch.int32, (B,))
        ids = self._dev(image_ids, "image_ids", torch.int32, (B,))
        xywh, area, score, cat = self._row_targets(B, s0, s1)
        self.image_ids[s0:s1].copy_(ids)
        N.coco_prop_rows(prop, pc, xywh, area, score, cat, xyxy_as_xywh=xyxy_as_xywh)
        N.coco_box_iou(xywh, pc, gb, gc, gi, out=self._iou[:B])
        self._match(B, s0, s1, pc, ga, gi, gk, gc)

    @torch.no_grad()
    def accumulate(self):
        """-> {'precision' [T, R, K, A, M], 'recall' [T, K, A, M], 'scores' [T, R, K, A, M]}: float64 device tensors of the evaluator
        (overwritten by the next call), COCOeval.eval's arrays over every image added so far (K = 1 with use_cats=False)"""
        self._require_images()
        N.coco_accumulate(self.image_ids, self.n_images, self.cat, self.rank, self.score, self.bits, self.npig, self.seen,
                          self.d_rec_thrs, self.d_max_dets, self.max_dets[-1], self.T, self.ws, self.precision, self.recall, self.scores)
        self._accumulated = self.n_images
        return {'precision': self.precision, 'recall': self.recall, 'scores': self.scores}

    @torch.no_grad()
    def summarize(self):
        """-> numpy float64 [12]: COCOeval.stats (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl), or for 'keypoints'
        [10]: (AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl); the one host wait"""
        self._ensure_accumulated()
        N.coco_summarize(self.precision, self.recall, (self.T, self.R, self.KE, self.A, self.M), self.d_specs, self.stats)
        stats = self.stats.cpu().numpy()
        self._check_merge_flags()
        return stats
