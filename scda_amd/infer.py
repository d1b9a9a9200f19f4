"""Batched, device-resident inference of a FasterRCNN_AdEx detector (VGG16, vgg16_bn, the ResNet-50 C4 detector).

The eval-mode forward (validate()) takes one round trip to the host per image for the RPN ranking and another for the box
prediction.  `predict` runs the same detector over B images with the test-time box logic on the device
(scda_amd/csrc/infer_ops.hip): backbone -> RPN -> objectness -> top-k, decode, NMS and a fixed-capacity gather of the proposals
-> RCNN head -> soft-max -> per-class decode, NMS and the per-image top_n.  Nothing in between waits for the host or allocates a
result buffer, so a fixed (B, H, W) batch can be recorded into one graph (`Predictor.capture`).  `rows` is the one call that
synchronises: it turns the device results into the row layout of the eval forward / validate().

Tie rules (include/scda_ops.h): RPN top-k by score, ties by ascending anchor index; per-class lists and the per-image top_n by
score, ties as numpy's argsort()[::-1] leaves them (later row first).  Where numpy's order is defined, the results are the eval
forward's; the RPN's exp of the size deltas is the correctly rounded float32 exp (numpy's is its own routine), so proposal
coordinates can differ from the eval forward's in their last bits.

Instance masks (opt-in, `Predictor(model, cfg, masks=True)`, the detector built with the mask branch): behind the box prediction the
detections become the mask head's RoIs, `model.mask_predictor` gives the per-class logits, each detection's own class plane goes through
the sigmoid and functions/mask.py:21-49 (`predict_masks`: the plane resized to the box as Pillow >= 7 resizes it, pasted into the image;
scda_amd/csrc/mask_ops.hip, bit for bit) runs on the device into bit-packed planes, bit = probability >= mask_threshold.  The paste is
pinned against the reference; the sigmoid and the 0.5 threshold are the Mask R-CNN definition and parity-unpinned (the reference's own
use of the heat map is in its missing models/mask_rcnn/mask_rcnn.py).  `mask_rows` turns the words into boolean arrays.

COCO results (opt-in on top, `Predictor(model, cfg, masks=True, rle=True)`): behind the paste every detection's plane is run-length encoded
on the device at its image's (h, w) (scda_amd/csrc/mask_rle.hip: pycocotools' rleEncode / rleToString / rleArea / rleToBbox bit for bit),
so what leaves the device is the result -- a few kilobytes per mask -- not the raster.  `segm_rows` is the call that waits and returns
the `{'size', 'counts'}` dictionaries; a mask with more runs than the device capacity is encoded on the host from its own plane
(scda_amd/mask_rle_host.py, the same rule) and counted.

Results at the original image size (opt-in on top, `Predictor(model, cfg, masks=True, original_size=(Ho, Wo))`, image_info rows
(h, w, resize_scale, origin_h, origin_w)): behind the paste every detection's float plane is resized once more to its image's
(origin_h, origin_w) as the reference's write_results_to_file does (tools/mask_rcnn_train_val.py:422, Pillow's resize bit for bit;
scda_amd/csrc/mask_rescale.hip, one fused kernel that never writes the float plane to memory) and thresholded there with `>` (:423)
into mask_bits_orig; det_orig holds the boxes divided by resize_scale (:408).  With rle=True the run-length results are those of
mask_bits_orig.  The limits (original sizes above (Ho, Wo), a down-scale above native.mask_rescale_max_ratio() = 4) are flagged per
image on the device; mask_rows and segm_rows raise for a flagged image.

Keypoints (opt-in, `Predictor(model, cfg, keypoints=True)`, the detector built with the keypoint branch; independent of `masks`): behind
the box prediction the detections become the keypoint head's RoIs, `model.keypoint_predictor` gives [B * top_n, Kp, 56, 56] heat maps and
scda_amd/csrc/keypoint_ops.hip turns them into (x, y, score) rows without writing an image-sized plane: each heat map resized to its
box as functions/mask.py:21-49 resizes a mask plane, then np.argmax over the part of the box inside the padded image.  The reference's own
heat-map decoder is in its missing models/mask_rcnn/mask_rcnn.py: the CHOICE OF THIS RULE IS OURS, and its parity is pinned to
predict_masks + np.argmax, not to a reference keypoint decoder (include/scda_ops.h).  Training the branch is the detector's (cfg['train_keypoint_target'],
ScdaTrainer.step(..., gt_keypoints=)), with targets that invert this decode.  Not covered: heat maps above 64 x 64, images of one call with different (h, w) in the host-side helpers (the Predictor decodes against the batch's padded shape)."""
import numpy as np
import torch

from scda_amd import device_boxes
from scda_amd import native as N


def _objectness(rpn_pred_cls):
    from scda_amd.dropin.models.faster_rcnn.faster_rcnn_adver_expansion_reweight_cluster import _objectness as obj
    return obj(rpn_pred_cls)


def _sections(cfg):
    """(rpn test cfg, predict cfg, shared) of an experiment cfg; the shared keys fill what a section leaves out"""
    shared = cfg.get('shared', {})
    rpn = dict(shared, **cfg['test_rpn_proposal_cfg'])
    box = dict(shared, **cfg['test_predict_bbox_cfg'])
    return rpn, box


class PredictorResult(tuple):
    """The output tuple of a Predictor pass.  Entries 0..3 are proposals, proposal_counts, detections, detection_counts; every option
    appends its entries behind them in the order masks (mask_bits), rle (the run-length dict, entry 5), original_size (mask_bits_orig
    int32 [B, top_n, Ho, ceil(Wo/32)], det_orig float32 [B, top_n, 7], orig_status int32 [B], 0 = fine, see include/scda_ops.h),
    keypoints (keypoints, keypoints_orig).  Every entry is also an attribute of the name in FIELDS; one the pass does not carry is None."""
    FIELDS = ('proposals', 'proposal_counts', 'detections', 'detection_counts', 'mask_bits', 'rle', 'mask_bits_orig', 'det_orig',
              'orig_status', 'keypoints', 'keypoints_orig')

    def __new__(cls, entries=(), names=()):
        self = super().__new__(cls, entries)
        self._names = dict(names)                           # name -> position (None: absent)
        return self

    def plus(self, **named):
        """this result with the named entries appended"""
        n = len(self)
        return PredictorResult(tuple(self) + tuple(named.values()), dict(self._names, **{k: n + i for i, k in enumerate(named)}))

    def __getattr__(self, name):
        at = self.__dict__.get('_names', {}).get(name)
        if at is not None:
            return self[at]
        if name in self.FIELDS:
            return None
        raise AttributeError(name)


OriginalSizeResult = PredictorResult                        # the name of the result of an original_size pass before every pass had one


def _need_pillow7(what):
    import PIL
    if int(PIL.__version__.split(".")[0]) < 7:
        raise ValueError("device %s path: Pillow %s resizes with NEAREST by default; the device path restates Pillow >= 7's BICUBIC "
                         "default -- use predict_%ss on the host" % (what, PIL.__version__, what))


def _check_status(status, what):
    flagged = [(b, int(v)) for b, v in enumerate(status.cpu().numpy().reshape(-1)) if v]
    if flagged:
        raise ValueError("%s: no original-size masks for images %s (image, status): 1 = the original size exceeds the Predictor's "
                         "original_size capacity, 2 = an original size below 1, 4 = a down-scale above %d, 8 = a bad (h, w)"
                         % (what, flagged, N.mask_rescale_max_ratio()))


class Predictor:
    """The buffers of one (B, H, W) shape on one device: proposals [B, P, 6], proposal_counts int32 [B], detections [B, top_n, 7],
    detection_counts int32 [B] and the kernels' workspaces, allocated on the first call and reused by every later one.

        pred = Predictor(model, cfg)
        out = pred(images, image_info)        # eager; the first call also re-packs weights and uploads the anchor grid
        pred.capture(images, image_info)      # after that first call: record one pass into a graph
        pred.images.copy_(...); pred.image_info.copy_(...); pred.replay()   # -> the same four tensors, refilled

    The returned tensors are the Predictor's own: a later call overwrites them.

    masks=True (a detector with the mask branch only): the result grows by mask_bits int32 [B, top_n, H, ceil(W/32)] at the batch's
    padded (H, W): bit (c % 32) of word c // 32 of row y = (mask probability at (y, c) >= mask_threshold); the planes of padding rows
    are zero.  One more fixed buffer per shape (13.4 MB per image for 100 detections at 800 x 1344), no additional wait for the host.

    rle=True (with masks=True): the result grows by ONE more element, a dict of device tensors per detection -- n_runs int32 [B, top_n]
    (the true run count; > the capacity = overflow), counts int32 [B, top_n, cap] (uint32 values), n_bytes int32 [B, top_n], chars uint8
    [B, top_n, cap * chars per count], area int32 [B, top_n], bbox int32 [B, top_n, 4] = (x, y, w, h) of the MASK as rleToBbox gives it,
    size int32 [B, 2] = the (h, w) every mask of the image was encoded at (image_info[b, 0:2], read on the device).  Padding detections
    carry the empty-mask code.  rle_capacity: runs kept per detection, default 4 * W (two segments per column on average over the whole
    width); a default, not a guarantee: segm_rows encodes an overflowing mask on the host.

    original_size=(Ho, Wo) (with masks=True; image_info [B, >= 5] = (h, w, resize_scale, origin_h, origin_w)): the capacity of the
    original-size planes.  The result (a PredictorResult, as of every pass) grows behind the entries above by mask_bits_orig int32
    [B, top_n, Ho, ceil(Wo/32)] -- bit = (the pasted float plane of the image's (h, w), resized by Pillow's rule to (origin_h, origin_w),
    > mask_threshold), zero outside origin_h x origin_w --, det_orig float32 [B, top_n, 7] = the detections with their box divided by
    resize_scale in float32, and orig_status int32 [B], non-zero for an image beyond the kernel's limits (its masks are empty).  With
    rle=True entry 5 holds the run-length results of mask_bits_orig, `size` = (origin_h, origin_w), rle_capacity defaulting to 4 * Wo.
    mask_bits (entry 4) stays the input-resolution plane with its `>=`.  One more fixed buffer, one more launch, no wait for the host.

    soft_nms={'method': 'linear' | 'gaussian' | 'hard', 'sigma': 0.5, 'Nt': 0.3, 'threshold': 0.001} (any subset; the reference's defaults
    fill the rest): the per-class lists go through cython_nms.soft_nms on the device (scda_amd/csrc/soft_nms.hip, bit for bit) in place
    of the hard NMS, and the per-image top_n ranks by the rescored scores -- the rows the eval forward gives with the same dict under
    test_predict_bbox_cfg's `soft_nms` key, which is also where this argument's default comes from (the argument overrides the key).
    None and no key: hard NMS, the bytes as ever.  ValueError for an unknown method, a sigma <= 0 or a post_nms_top_n above the kernel's
    capacity of 2048 rows per list.  The RPN stage keeps its hard NMS.

    keypoints=True (a detector with the keypoint branch only; image_info [B, >= 3] = (h, w, resize_scale, ...); independent of masks):
    the result grows by TWO entries, appended after every other one: keypoints float32 [B, top_n, Kp, 3] = (x, y, score) per detection
    and keypoint at the network input's coordinates (the rule: include/scda_ops.h, scda_keypoint_decode_hip; score = the raw resized
    heat-map value), and keypoints_orig, the same with x and y divided in float32 by resize_scale (tools/mask_rcnn_train_val.py:417, as
    det_orig divides its boxes).  Rows of padding detections are zero.  The two are also named: .keypoints, .keypoints_orig.  The
    heat maps the decode read stay reachable as `pred.keypoint_heat` ([B * top_n, Kp, 56, 56], a view) until the
    next pass.  Fixed buffers per shape, two more launches behind the head, no additional wait for the host."""

    def __init__(self, model, cfg, masks=False, mask_threshold=0.5, rle=False, rle_capacity=None, soft_nms=None, original_size=None,
                 keypoints=False):
        if model.training:
            raise ValueError("Predictor: put the detector in eval mode first (model.eval())")
        self.masks, self.mask_threshold = bool(masks), float(mask_threshold)
        self.rle, self.rle_capacity = bool(rle), None if rle_capacity is None else int(rle_capacity)
        if self.rle and not self.masks:
            raise ValueError("Predictor: rle=True encodes the instance masks; it needs masks=True")
        if self.rle_capacity is not None and self.rle_capacity < 1:
            raise ValueError("Predictor: rle_capacity must be >= 1")
        self.original_size = None if original_size is None else (int(original_size[0]), int(original_size[1]))
        if self.original_size is not None:
            if not self.masks:
                raise ValueError("Predictor: original_size resizes the instance masks; it needs masks=True")
            if min(self.original_size) < 1:
                raise ValueError("Predictor: original_size = (Ho, Wo) must be >= 1")
        if self.masks:
            if not getattr(model, 'with_mask', False):
                raise ValueError("Predictor: masks=True needs a detector with the mask branch (cfg with_mask)")
            _need_pillow7("mask")
        self.keypoints = bool(keypoints)
        if self.keypoints:
            if not getattr(model, 'with_keypoint', False):
                raise ValueError("Predictor: keypoints=True needs a detector with the keypoint branch (cfg with_keypoint)")
            _need_pillow7("keypoint")
        self.keypoint_heat = None
        self.model, self.cfg = model, cfg
        self.rpn_cfg, self.box_cfg = _sections(cfg)
        if not self.box_cfg.get('bbox_normalize_stats_precomputed', False):
            raise ValueError("Predictor: the device box prediction decodes de-normalised deltas "
                             "(bbox_normalize_stats_precomputed = true); this cfg does not")
        if int(self.box_cfg['top_n']) <= 0:
            raise ValueError("Predictor: test_predict_bbox_cfg.top_n must be > 0 (the detections have a fixed capacity)")
        # soft-NMS in place of the per-class hard NMS: the explicit argument, else test_predict_bbox_cfg's optional `soft_nms` key
        self.soft_nms = N.soft_nms_setting(soft_nms if soft_nms is not None else self.box_cfg.get('soft_nms'))
        if self.soft_nms is not None and int(self.rpn_cfg['post_nms_top_n']) > N.soft_nms_capacity():
            raise ValueError("Predictor: soft_nms holds a class list of at most %d rows; test_rpn_proposal_cfg.post_nms_top_n is %d"
                             % (N.soft_nms_capacity(), int(self.rpn_cfg['post_nms_top_n'])))
        self.shape = None
        self.images = self.image_info = None
        self.graph = None
        self._out = None

    def _allocate(self, B, fh, fw, A, C, dev):
        P, top_n = int(self.rpn_cfg['post_nms_top_n']), int(self.box_cfg['top_n'])
        if P <= 0:
            raise ValueError("Predictor: test_rpn_proposal_cfg.post_nms_top_n must be > 0 (the proposals have a fixed capacity)")
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.P, self.top_n = P, top_n
        self.rois = torch.zeros(B * P, 5, **f32)
        self.props = torch.zeros(B * P, 6, **f32)
        self.counts = torch.zeros(B, **i32)
        self.det = torch.zeros(B, top_n, 7, **f32)
        self.det_counts = torch.zeros(B, **i32)
        self.rpn_ws = torch.empty(max(N.rpn_proposals_workspace_bytes(B, A, fh, fw, int(self.rpn_cfg['pre_nms_top_n'])), 8), **u8)
        self.box_ws = torch.empty(max(N.box_predict_workspace_bytes(B, P, C), 8), **u8)
        self.anchors64 = device_boxes.anchors_on_device(fh, fw, self.rpn_cfg, dev)[1]

    def _allocate_masks(self, B, H, W, dev):
        R = B * self.top_n
        self.mask_rois = torch.zeros(R, 5, dtype=torch.float32, device=dev)
        self.mask_cls = torch.zeros(R, dtype=torch.int32, device=dev)
        self.mask_planes = None                                               # [R, h, w] once the head's output size is known
        self.mask_bits = torch.zeros(B, self.top_n, H, (W + 31) // 32, dtype=torch.int32, device=dev)

    def _allocate_keypoints(self, B, W, dev):
        R, Kp = B * self.top_n, int(self.model.num_keypoints)
        self.kp_rois = torch.zeros(R, 5, dtype=torch.float32, device=dev)
        self.kp_cls = torch.zeros(R, dtype=torch.int32, device=dev)
        self.kp_out = torch.zeros(B, self.top_n, Kp, 3, dtype=torch.float32, device=dev)
        self.kp_out_orig = torch.zeros(B, self.top_n, Kp, 3, dtype=torch.float32, device=dev)
        self.kp_ws = torch.empty(max(N.keypoint_decode_workspace_bytes(R, Kp, W), 8), dtype=torch.uint8, device=dev)

    def _keypoints(self, feat, info, B, H, W):
        """detections -> RoIs -> keypoint head -> each heat map's first maximum inside its resized window; x and y / resize_scale"""
        N.det_rois(self.det, self.det_counts, self.kp_rois, self.kp_cls)
        heat = self.model.keypoint_predictor(feat, self.kp_rois).detach()
        if heat.shape[1] != self.kp_out.shape[2]:
            raise ValueError("Predictor: the keypoint head gives %d maps, model.num_keypoints is %d" % (heat.shape[1], self.kp_out.shape[2]))
        self.keypoint_heat = heat
        N.keypoint_decode(self.kp_rois, heat, H, W, cls=self.kp_cls, out=self.kp_out.view(B * self.top_n, -1, 3), ws=self.kp_ws)
        self.kp_out_orig.copy_(self.kp_out)
        self.kp_out_orig[:, :, :, 0:2].div_(info[:, 2].view(B, 1, 1, 1))
        return self.kp_out, self.kp_out_orig

    def _allocate_orig(self, B, dev):
        Ho, Wo = self.original_size
        R = B * self.top_n
        self.mask_bits_orig = torch.zeros(B, self.top_n, Ho, (Wo + 31) // 32, dtype=torch.int32, device=dev)
        self.det_orig = torch.zeros(B, self.top_n, 7, dtype=torch.float32, device=dev)
        self.foot_rois = torch.zeros(R, 5, dtype=torch.float32, device=dev)
        self.orig_status = torch.zeros(B, dtype=torch.int32, device=dev)

    def _orig(self, info, B, H, W):
        """behind _masks: every detection's pasted plane resized to its image's original size and thresholded there; the boxes divided
        by resize_scale"""
        Ho, Wo = self.original_size
        N.mask_rescale(self.mask_rois, self.mask_planes, H, W, info, Ho, Wo, cls=self.mask_cls, packed=True,
                       threshold=self.mask_threshold, out=self.mask_bits_orig.view(B * self.top_n, Ho, -1), foot_rois=self.foot_rois,
                       status=self.orig_status)
        self.det_orig.copy_(self.det)
        self.det_orig[:, :, 1:5].div_(info[:, 2].view(B, 1, 1))

    def _rle_orig(self, info, B):
        """the run-length code of mask_bits_orig at (origin_h, origin_w); the footprints limit the columns read (outside its footprint
        a plane is 0.0, which is not > a threshold >= 0)"""
        Ho, Wo = self.original_size
        N.mask_rle(self.mask_bits_orig.view(B * self.top_n, Ho, -1), image_info=info, info_column=3,
                   rois=self.foot_rois if self.mask_threshold >= 0 else None, cap_runs=self.rle_cap, ws=self.rle_ws, out=self.rle_flat)
        size = self.rle_out['size']
        size.copy_(info[:, 3:5])
        size[:, 0].clamp_(1, Ho)
        size[:, 1].clamp_(1, 32 * ((Wo + 31) // 32))
        return self.rle_out

    def _allocate_rle(self, B, H, W, dev):
        R, Wd = B * self.top_n, (W + 31) // 32
        cap = 4 * W if self.rle_capacity is None else self.rle_capacity
        i32 = dict(dtype=torch.int32, device=dev)
        self.rle_cap = cap
        self.rle_ws = torch.empty(max(N.mask_rle_workspace_bytes(R, H, Wd, cap), 8), dtype=torch.uint8, device=dev)
        self.rle_flat = {'n_runs': torch.zeros(R, **i32), 'counts': torch.zeros(R, cap, **i32), 'n_bytes': torch.zeros(R, **i32),
                         'chars': torch.zeros(R, cap * N.mask_rle_max_chars(H, 32 * Wd), dtype=torch.uint8, device=dev),
                         'area': torch.zeros(R, **i32), 'bbox': torch.zeros(R, 4, **i32)}
        self.rle_out = {k: v.view(B, self.top_n, *v.shape[1:]) for k, v in self.rle_flat.items()}
        self.rle_out['size'] = torch.zeros(B, 2, **i32)

    def _rle(self, info, B, H, W):
        """every detection's packed plane -> its run-length code at the image's (h, w); the paste's windows limit the columns read
        (valid for a positive threshold: outside its window a pasted plane is 0.0)"""
        N.mask_rle(self.mask_bits.view(B * self.top_n, H, -1), image_info=info,
                   rois=self.mask_rois if self.mask_threshold > 0 else None, cap_runs=self.rle_cap, ws=self.rle_ws, out=self.rle_flat)
        size = self.rle_out['size']
        size.copy_(info[:, :2])                                               # float32 -> int32 truncates like the kernel
        size[:, 0].clamp_(1, H)
        size[:, 1].clamp_(1, 32 * ((W + 31) // 32))
        return self.rle_out

    def _masks(self, feat, B, H, W):
        """detections -> RoIs -> mask head -> own class plane through the sigmoid -> resized, pasted and packed"""
        N.det_rois(self.det, self.det_counts, self.mask_rois, self.mask_cls)
        logits = self.model.mask_predictor(feat, self.mask_rois).detach()
        R, _, h, w = logits.shape
        if self.mask_planes is None or self.mask_planes.shape != (R, h, w):
            self.mask_planes = torch.empty(R, h, w, dtype=torch.float32, device=logits.device)
        N.mask_select(logits, self.mask_cls, sigmoid=True, out=self.mask_planes)
        N.mask_paste(self.mask_rois, self.mask_planes, H, W, cls=self.mask_cls, packed=True, threshold=self.mask_threshold,
                     out=self.mask_bits.view(R, H, -1))
        return self.mask_bits

    def _info(self, image_info, B, dev):
        if torch.is_tensor(image_info) and image_info.is_cuda and image_info.dtype == torch.float32 and image_info.is_contiguous():
            return image_info
        info = torch.as_tensor(np.asarray(image_info.cpu() if torch.is_tensor(image_info) else image_info, dtype=np.float32))
        if self.image_info is None or self.image_info.shape != info.shape:
            self.image_info = torch.empty(info.shape, dtype=torch.float32, device=dev)
        self.image_info.copy_(info)
        return self.image_info

    @torch.no_grad()
    def __call__(self, images, image_info):
        model, rc, bc = self.model, self.rpn_cfg, self.box_cfg
        B = images.shape[0]
        dev = images.device
        info = self._info(image_info, B, dev)
        if info.shape[0] != B or info.shape[1] < 2:
            raise ValueError("Predictor: image_info must be [B, >=2] (h, w, ...)")
        if self.original_size is not None and info.shape[1] < 5:
            raise ValueError("Predictor: original_size needs image_info [B, >=5] (h, w, resize_scale, origin_h, origin_w)")
        if self.keypoints and info.shape[1] < 3:
            raise ValueError("Predictor: keypoints=True needs image_info [B, >=3] (h, w, resize_scale, ...)")
        feat = model.feature_extractor(images)
        rpn_cls, rpn_loc = model.rpn(feat)
        prob = _objectness(rpn_cls).contiguous()
        loc = rpn_loc.detach().contiguous()
        _, A4, fh, fw = loc.shape
        shape = (tuple(images.shape), str(dev), A4, fh, fw)
        if self.shape != shape:
            C = int(self.box_cfg['num_classes'])
            self._allocate(B, fh, fw, A4 // 4, C, dev)
            if self.masks:
                self._allocate_masks(B, images.shape[2], images.shape[3], dev)
            if self.original_size is not None:
                self._allocate_orig(B, dev)
            if self.rle:
                self._allocate_rle(B, *(self.original_size or images.shape[2:]), dev)
            if self.keypoints:
                self._allocate_keypoints(B, images.shape[3], dev)
            self.shape = shape
            self.graph = None
        N.rpn_proposals_batched(prob, loc, self.anchors64, info, int(rc['pre_nms_top_n']), float(rc['roi_min_size']),
                                float(rc['nms_iou_thresh']), self.P, self.rpn_ws, self.rois, self.props, self.counts)
        _, cls, bloc = model.rcnn(feat, self.rois)
        cprob = N.row_softmax(cls.detach().contiguous())
        if cprob.shape[1] * 4 != bloc.shape[1] or cprob.shape[1] != int(bc['num_classes']):
            raise ValueError("Predictor: the head's class count differs from cfg num_classes")
        N.box_predict(self.rois, self.counts, cprob, bloc.detach().contiguous(), info, bc['bbox_normalize_stds'],
                      bc['bbox_normalize_means'], float(bc['score_thresh']), float(bc['nms_iou_thresh']), self.top_n, self.box_ws,
                      self.det, self.det_counts, soft_nms=self.soft_nms)
        H, W = images.shape[2:]
        out = PredictorResult().plus(proposals=self.props.view(B, self.P, 6), proposal_counts=self.counts, detections=self.det,
                                     detection_counts=self.det_counts)
        if self.masks:
            out = out.plus(mask_bits=self._masks(feat, B, H, W))
        if self.original_size is not None:
            self._orig(info, B, H, W)
            if self.rle:
                out = out.plus(rle=self._rle_orig(info, B))
            out = out.plus(mask_bits_orig=self.mask_bits_orig, det_orig=self.det_orig, orig_status=self.orig_status)
        elif self.rle:
            out = out.plus(rle=self._rle(info, B, H, W))
        if self.keypoints:
            kp, kp_orig = self._keypoints(feat, info, B, H, W)
            out = out.plus(keypoints=kp, keypoints_orig=kp_orig)
        self._out = out
        return out

    def capture(self, images, image_info):
        """record one pass over static copies of (images, image_info) into a graph (call once eagerly first); returns the outputs"""
        if self._out is None:
            raise RuntimeError("Predictor.capture: run one eager call first (it re-packs weights and allocates the buffers)")
        self.images = images.detach().clone()
        info = self._info(image_info, images.shape[0], images.device)
        if info is not self.image_info:
            self.image_info = info.clone()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self(self.images, self.image_info)
        return self._out

    def replay(self):
        if self.graph is None:
            raise RuntimeError("Predictor.replay: nothing captured")
        self.graph.replay()
        return self._out


_PREDICTORS = {}


def predict(model, images, image_info, cfg, masks=False, mask_threshold=0.5, rle=False, rle_capacity=None, soft_nms=None,
            original_size=None, keypoints=False):
    """images [B,3,H,W] on the device, image_info [B,>=2] (host or device) -> device tensors
    (proposals [B,P,6] = (b, x1, y1, x2, y2, score), proposal_counts int32 [B], detections [B,top_n,7] =
    (b, x1, y1, x2, y2, score, class), detection_counts int32 [B]); rows past an image's count are padding.
    masks=True: a fifth tensor, mask_bits int32 [B,top_n,H,ceil(W/32)] (see Predictor); rle=True on top: a sixth element, the dict of
    run-length results (see Predictor, segm_rows).
    soft_nms: see Predictor (a dict; None = the cfg's own `soft_nms` key, if any).
    original_size=(Ho, Wo): see Predictor; three more entries, mask_bits_orig, det_orig and orig_status (image_info [B,>=5]).
    keypoints=True: see Predictor; two more entries at the end, keypoints and keypoints_orig float32 [B,top_n,Kp,3] (image_info [B,>=3]).
    The result is a PredictorResult: the tuple above, every entry also reachable by name.
    One Predictor per (model, cfg, masks, mask_threshold with masks, rle, rle_capacity with rle, soft_nms, original_size, keypoints) is
    kept and reused; its buffers are overwritten by the next call."""
    key = (id(model), id(cfg), bool(masks), float(mask_threshold) if masks else None, bool(rle), rle_capacity if rle else None,
           None if soft_nms is None else N.soft_nms_setting(soft_nms),
           None if original_size is None else (int(original_size[0]), int(original_size[1])), bool(keypoints))
    p = _PREDICTORS.get(key)
    if p is None or p.model is not model:
        p = _PREDICTORS[key] = Predictor(model, cfg, masks=masks, mask_threshold=mask_threshold, rle=rle, rle_capacity=rle_capacity,
                                         soft_nms=soft_nms, original_size=original_size, keypoints=keypoints)
    return p(images, image_info)


def rows(proposals, proposal_counts, detections, detection_counts):
    """device results -> (proposals float32 [n,6], detections float32 [m,7]) in the eval forward's layout: images in order, each
    image's real rows only.  The one call of this module that waits for the device."""
    p, pc, d, dc = (t.cpu().numpy() for t in (proposals, proposal_counts, detections, detection_counts))
    props = np.concatenate([p[b, :pc[b]] for b in range(p.shape[0])], 0).reshape(-1, 6)
    dets = np.concatenate([d[b, :dc[b]] for b in range(d.shape[0])], 0).reshape(-1, 7)
    return props, dets


def mask_rows(mask_bits, detection_counts, width=None, status=None):
    """mask_bits [B, top_n, H, ceil(W/32)] + detection_counts [B] -> a list of B boolean arrays [n_b, H, W]: each image's real
    detections in `rows`' order.  width: W when it is not a multiple of 32 (default: every stored column).  Like `rows`, this waits for
    the device.  status: the orig_status of a Predictor(original_size=...) pass when mask_bits is its mask_bits_orig (every image's rows
    are then [n_b, Ho, Wo]: crop them to the image's own (origin_h, origin_w)); ValueError for a flagged image."""
    if status is not None:
        _check_status(status, "mask_rows")
    words = mask_bits.cpu().numpy().view(np.uint32)
    counts = detection_counts.cpu().numpy()
    B, _, H, Wd = words.shape
    W = Wd * 32 if width is None else int(width)
    if not 0 < W <= Wd * 32:
        raise ValueError("mask_rows: width must be in (0, %d]" % (Wd * 32))
    out = []
    for b in range(B):
        w = np.ascontiguousarray(words[b, :int(counts[b])])
        bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder='little')        # [n, H, Wd * 32]: bit j of a word = column 32 i + j
        out.append(bits[:, :, :W].astype(bool))
    return out


def pack_masks(masks):
    """bool [N, H, W] (host) -> int32 words [N, H, ceil(W/32)], bit (c % 32) of word c // 32 = masks[n, y, c]: the layout of mask_bits
    and the inverse of mask_rows' unpacking, so that ground-truth masks can be given to native.mask_iou / native.mask_rle"""
    m = np.asarray(masks, dtype=bool)
    if m.ndim != 3:
        raise ValueError("pack_masks: masks must be [N, H, W]")
    n, H, W = m.shape
    Wd = (W + 31) // 32
    padded = np.zeros((n, H, Wd * 32), dtype=np.uint8)
    padded[:, :, :W] = m
    words = np.packbits(padded, axis=-1, bitorder='little').reshape(n, H, Wd, 4)
    words = (words[..., 0].astype(np.uint32) | (words[..., 1].astype(np.uint32) << 8) | (words[..., 2].astype(np.uint32) << 16)
             | (words[..., 3].astype(np.uint32) << 24))
    return torch.from_numpy(words.view(np.int32))


def segm_rows(out, with_fallbacks=False):
    """the result of a Predictor(masks=True, rle=True) pass -> per image a list with one dict per real detection, in `rows`' order:
    {'size': [h, w], 'counts': str, 'area': int, 'bbox': [x, y, w, h]} -- 'size' and 'counts' are pycocotools' compressed RLE of the mask
    at the network-input resolution, 'area' / 'bbox' its rleArea / rleToBbox.  A detection whose run count exceeded the device capacity
    is encoded here from its own plane of mask_bits by scda_amd.mask_rle_host (the same rule, the same bytes); their number is logged and,
    with with_fallbacks=True, returned as a second value.  This call waits for the device.  What crosses to the host: 28 bytes per
    detection slot, 12 per image, each image's strings (its real detections x the longest of them) and one plane per fallback.
    The result of a pass with original_size (it carries mask_bits_orig): the same at the ORIGINAL image size -- 'size' = [origin_h,
    origin_w], the masks those of mask_bits_orig; ValueError for an image whose orig_status is set."""
    import logging
    from scda_amd import mask_rle_host
    det_counts, mask_bits, rle = out[3], out[4], out[5]
    if getattr(out, 'mask_bits_orig', None) is not None:
        if out.rle is None:
            raise ValueError("segm_rows: the pass has no run-length results (Predictor(rle=True))")
        _check_status(out.orig_status, "segm_rows")
        mask_bits = out.mask_bits_orig
    dc = det_counts.cpu().numpy()
    n_runs, n_bytes, area = (rle[k].cpu().numpy() for k in ('n_runs', 'n_bytes', 'area'))
    bbox, size = rle['bbox'].cpu().numpy(), rle['size'].cpu().numpy()
    cap = rle['counts'].shape[2]
    res, fallbacks = [], 0
    for b in range(dc.shape[0]):
        n = int(dc[b])
        h, w = int(size[b, 0]), int(size[b, 1])
        over = n_runs[b, :n] > cap
        longest = int(n_bytes[b, :n][~over].max()) if n and not over.all() else 0
        chars = rle['chars'][b, :n, :longest].cpu().numpy() if longest else None
        rows_b = []
        for j in range(n):
            if over[j]:
                plane = mask_bits[b, j].cpu().numpy().view(np.uint32)
                bits = np.unpackbits(np.ascontiguousarray(plane).view(np.uint8), axis=-1, bitorder='little')
                rows_b.append(mask_rle_host.encode(bits[:h, :w].astype(bool)))
                fallbacks += 1
            else:
                rows_b.append({'size': [h, w], 'counts': chars[j, :n_bytes[b, j]].tobytes().decode('ascii'),
                               'area': int(area[b, j].view(np.uint32)), 'bbox': [int(v) for v in bbox[b, j].view(np.uint32)]})
        res.append(rows_b)
    if fallbacks:
        logging.getLogger('global').info("segm_rows: %d masks exceeded the device run capacity of %d and were encoded on the host"
                                         % (fallbacks, cap))
    return (res, fallbacks) if with_fallbacks else res
