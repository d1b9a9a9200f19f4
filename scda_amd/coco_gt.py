"""COCO ground truth for scda_amd.coco_eval.CocoEvaluator from annotation dicts: what COCO.annToMask (reference
datasets/pycocotools/coco.py:411-439, _mask.pyx frPoly / frUncompressedRLE / decode) builds on the host as one dense h x w byte image per
instance is rasterised on the MI355X by scda_mask_frpoly_hip (include/scda_ops.h states the rule) straight into the packed planes
CocoEvaluator.add takes as gt_mask_bits.  Only vertices and run counts cross to the device.

flatten_annotations() is the host half (numpy): it lays the annotations of a batch out as the flat arrays of the entry point and checks
every limit the kernels rely on.  GroundTruth owns the device buffers and makes the call.

NOT covered: boxes as segmentations (frBbox / rleFrBbox -- a polygon list whose first entry has four values is what the reference reads
as boxes; it is refused here), the resize of ground-truth masks for training (datasets/coco_dataset.py:200).  Keypoint annotations are
carried as they stand (flatten_annotations(keypoints=True)) for CocoEvaluator(K, 'keypoints', num_keypoints=Kp); GroundTruth.load does not take them."""
import numpy as np
import torch

from scda_amd import native as N

MAX_COORD = 65535


def counts_from_string(s):
    """rleFrString (maskApi.c:217-230): a compressed `counts` string (str or bytes) -> uint32 counts.  Six bits per character, five of
    them payload; the last character's bit 0x10 extends the sign; from the fourth count on a value is a difference to the count two
    places before, which has itself been summed already."""
    if isinstance(s, str):
        s = s.encode('utf8')
    cnts, p, n = [], 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError("counts string ends inside a value")
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        if not 0 <= x < 2 ** 32:
            raise ValueError("counts string decodes to a run of %d pixels" % x)
        cnts.append(x)
    return np.asarray(cnts, dtype=np.uint32)


def _check_plane(H, Wd, n_planes):
    if not (1 <= H <= 65535 and Wd >= 1 and H * 32 * Wd < 2 ** 31 and n_planes <= 65535):
        raise ValueError("ground-truth planes: at most 65535 planes x 65535 rows and fewer than 2^31 pixels (got %d x [%d, %d])"
                         % (n_planes, H, Wd))


def flatten_annotations(per_image_anns, sizes, gcap, plane=None, keypoints=False, num_keypoints=None):
    """per_image_anns: per image a list of COCO annotation dicts -- 'segmentation' (a list of polygons [x0, y0, x1, y1, ...],
    {'size': [h, w], 'counts': list} or {'size': [h, w], 'counts': str | bytes}), 'bbox' [x, y, w, h], 'area', 'iscrowd', 'category_id';
    sizes: one (h, w) or one per image; gcap: the ground-truth slots per image.  Annotation g of image b becomes plane b * gcap + g.
    -> dict of host arrays: xy float64 [V, 2], poly_first int32 [P + 1], poly_plane int32 [P], rle_counts uint32 [C], rle_first int32
    [Q + 1], rle_plane int32 [Q], sizes int32 [B * gcap, 2] (scda_mask_frpoly_hip's inputs) and gt_boxes float64 [B, gcap, 4], gt_areas
    float64 [B, gcap] (the annotation's 'area' field, as COCOeval uses it), gt_iscrowd uint8, gt_categories int32 [B, gcap], gt_counts
    int32 [B] (CocoEvaluator.add's).

    The reference's skips are kept: a polygon contributes int(len(p) / 2) vertices (a trailing odd value is dropped), an annotation with
    no polygon is an empty mask.  ValueError -- before anything reaches the device -- for: more than gcap annotations in an image; sizes
    below 1 or, with plane = (H, Wd), outside the planes, and planes beyond the kernel's limits; a coordinate that is not finite or
    beyond +-65535; an RLE whose 'size' is not the image's or whose counts sum to more than h * w (the reference writes past its buffer
    there); a polygon list whose first entry has four values or fewer (the reference reads those as boxes, or refuses them).

    keypoints=True: the dict also holds gt_keypoints float64 [B, gcap, Kp, 3] (x, y, v) and gt_num_keypoints int32 [B, gcap] -- the
    annotations' 'keypoints' (3 Kp values, the same Kp in every annotation) and 'num_keypoints' fields, each as it stands (the
    evaluator reads both, as the reference does); an annotation without either, or with another length, raises ValueError.  Kp is
    num_keypoints if given (every annotation must then hold 3 * num_keypoints values), else that of the first annotation -- a batch
    without any annotation then raises, so a loader that may meet one passes num_keypoints."""
    B = len(per_image_anns)
    gcap = int(gcap)
    sz = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    if len(sz) == 1:
        sz = np.repeat(sz, B, axis=0)
    if len(sz) != B or gcap < 1:
        raise ValueError("flatten_annotations: sizes must be one (h, w) or one per image, gcap >= 1")
    if B and sz.min() < 1:
        raise ValueError("flatten_annotations: image sizes must be at least 1 x 1")
    if plane is not None:
        H, Wd = int(plane[0]), int(plane[1])
        _check_plane(H, Wd, B * gcap)
        if B and (sz[:, 0].max() > H or sz[:, 1].max() > 32 * Wd):
            raise ValueError("flatten_annotations: image sizes must lie inside the %d x %d planes" % (H, 32 * Wd))
    xy, poly_first, poly_plane = [], [0], []
    counts, rle_first, rle_plane = [], [0], []
    gt_boxes = np.zeros((B, gcap, 4), np.float64)
    gt_areas = np.zeros((B, gcap), np.float64)
    gt_iscrowd = np.zeros((B, gcap), np.uint8)
    gt_categories = np.zeros((B, gcap), np.int32)
    gt_counts = np.zeros(B, np.int32)
    gt_keypoints, gt_num_keypoints = None, np.zeros((B, gcap), np.int32)
    if num_keypoints is not None:
        if not keypoints or int(num_keypoints) < 1:
            raise ValueError("flatten_annotations: num_keypoints (>= 1) goes with keypoints=True")
        gt_keypoints = np.zeros((B, gcap, int(num_keypoints), 3), np.float64)
    for b, anns in enumerate(per_image_anns):
        if len(anns) > gcap:
            raise ValueError("flatten_annotations: image %d has %d annotations, gcap = %d" % (b, len(anns), gcap))
        h, w = int(sz[b, 0]), int(sz[b, 1])
        gt_counts[b] = len(anns)
        for g, ann in enumerate(anns):
            gt_boxes[b, g] = ann['bbox']
            gt_areas[b, g], gt_iscrowd[b, g], gt_categories[b, g] = ann['area'], ann.get('iscrowd', 0), ann['category_id']
            if keypoints:
                if 'keypoints' not in ann or 'num_keypoints' not in ann:
                    raise ValueError("flatten_annotations: image %d annotation %d has no 'keypoints' / 'num_keypoints'" % (b, g))
                kp = np.asarray(ann['keypoints'], dtype=np.float64).reshape(-1)
                if gt_keypoints is None:
                    if len(kp) == 0 or len(kp) % 3:
                        raise ValueError("flatten_annotations: image %d annotation %d: 'keypoints' must hold 3 Kp values" % (b, g))
                    gt_keypoints = np.zeros((B, gcap, len(kp) // 3, 3), np.float64)
                if len(kp) != gt_keypoints.shape[2] * 3:
                    raise ValueError("flatten_annotations: image %d annotation %d: %d keypoint values, %d in the first annotation"
                                     % (b, g, len(kp), gt_keypoints.shape[2] * 3))
                gt_keypoints[b, g] = kp.reshape(-1, 3)
                gt_num_keypoints[b, g] = ann['num_keypoints']
            segm = ann['segmentation']
            n = b * gcap + g
            if isinstance(segm, (list, tuple)):
                if len(segm) and len(segm[0]) <= 4:
                    raise ValueError("flatten_annotations: image %d annotation %d: a first polygon of %d values is a box or nothing to "
                                     "the reference (frBbox is not covered)" % (b, g, len(segm[0])))
                for p in segm:
                    v = np.asarray(p, dtype=np.float64).reshape(-1)
                    v = v[:2 * int(len(v) / 2)].reshape(-1, 2)
                    if not (np.isfinite(v).all() and (np.abs(v) <= MAX_COORD).all()):
                        raise ValueError("flatten_annotations: image %d annotation %d: coordinates must be finite and within +-%d"
                                         % (b, g, MAX_COORD))
                    xy.append(v)
                    poly_first.append(poly_first[-1] + len(v))
                    poly_plane.append(n)
            else:
                if tuple(int(v) for v in segm['size']) != (h, w):
                    raise ValueError("flatten_annotations: image %d annotation %d: RLE of size %s in an image of %s"
                                     % (b, g, list(segm['size']), [h, w]))
                c = segm['counts']
                if isinstance(c, (str, bytes)):
                    c = counts_from_string(c)
                c = np.asarray(c, dtype=np.int64).reshape(-1)
                if len(c) and c.min() < 0 or int(c.sum()) > h * w:
                    raise ValueError("flatten_annotations: image %d annotation %d: counts must be non-negative and sum to at most h * w = %d"
                                     % (b, g, h * w))
                counts.append(c.astype(np.uint32))
                rle_first.append(rle_first[-1] + len(c))
                rle_plane.append(n)
    i32 = lambda a: np.asarray(a, dtype=np.int32)                             # noqa: E731
    flat = {'xy': np.concatenate(xy).reshape(-1, 2) if xy else np.zeros((0, 2), np.float64),
            'poly_first': i32(poly_first), 'poly_plane': i32(poly_plane),
            'rle_counts': np.concatenate(counts) if counts else np.zeros(0, np.uint32),
            'rle_first': i32(rle_first), 'rle_plane': i32(rle_plane),
            'sizes': np.repeat(sz, gcap, axis=0).astype(np.int32),
            'gt_boxes': gt_boxes, 'gt_areas': gt_areas, 'gt_iscrowd': gt_iscrowd, 'gt_categories': gt_categories, 'gt_counts': gt_counts}
    if keypoints:
        if gt_keypoints is None:
            raise ValueError("flatten_annotations: keypoints=True takes Kp from the first annotation and there is none; pass num_keypoints")
        flat['gt_keypoints'], flat['gt_num_keypoints'] = gt_keypoints, gt_num_keypoints
    return flat


class GroundTruth:
    """The device side of the ground truth of one loader: gcap slots per image in planes [H, Wd] -- the Predictor's mask_bits planes, or
    with Predictor(original_size=(Ho, Wo)) its mask_bits_orig planes [Ho, ceil(Wo/32)], where COCO's annotations stand at their own
    coordinates and need no rescaling.
    load() uploads the flat arrays of a batch through native.upload and rasterises them with one scda_mask_frpoly_hip call; the plane
    and workspace buffers are kept and grow only when a batch needs more, so a steady loader allocates nothing but the small uploads.
    The returned tensors are the evaluator's until the next load()."""

    def __init__(self, device, gcap, H, Wd):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise N.ScdaNativeError("GroundTruth needs a HIP device; there is no CPU path")
        self.gcap, self.H, self.Wd = int(gcap), int(H), int(Wd)
        _check_plane(self.H, self.Wd, self.gcap)
        self._bits = self._area = self._ws = None
        self.mask_areas = None                  # int32 [B, gcap] of the last load(): the set pixels of every plane (rleArea)

    def load(self, per_image_anns, sizes):
        """-> (gt_boxes, gt_areas, gt_iscrowd, gt_categories, gt_counts, gt_mask_bits): the ground-truth arguments of CocoEvaluator.add,
        on the device.  No wait for the host."""
        f = flatten_annotations(per_image_anns, sizes, self.gcap, plane=(self.H, self.Wd))
        B, n = len(per_image_anns), len(per_image_anns) * self.gcap
        if n == 0:
            raise ValueError("GroundTruth.load: no image")
        dev = self.device
        if self._bits is None or self._bits.shape[0] < n:
            self._bits = torch.empty(n, self.H, self.Wd, dtype=torch.int32, device=dev)
            self._area = torch.empty(n, dtype=torch.int32, device=dev)
        need = N.mask_frpoly_workspace_bytes(len(f['poly_plane']), len(f['rle_plane']), self.H, self.Wd)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        d = {k: N.upload(v.view(np.int32) if v.dtype == np.uint32 else v, dev) for k, v in f.items()}
        bits, area = self._bits[:n], self._area[:n]
        N.mask_frpoly(d['xy'], d['poly_first'], d['poly_plane'], d['rle_counts'], d['rle_first'], d['rle_plane'], d['sizes'], self._ws,
                      bits, area=area)
        self.mask_areas = area.view(B, self.gcap)
        return (d['gt_boxes'], d['gt_areas'], d['gt_iscrowd'], d['gt_categories'], d['gt_counts'],
                bits.view(B, self.gcap, self.H, self.Wd))
