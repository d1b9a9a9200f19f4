"""Validation pass of the detector -- the contract of validate() / validate_single()
(reference tools/faster_rcnn_train_val.py:773-884 / 886-981): run the model in eval mode over a loader, count the RPN
recall at IoU 0.5, write `results.txt.rank<r>` rows `image_id x1 y1 x2 y2 score class` (top 100 detections per
image, clipped, divided by the resize scale), then score them with utils.cal_mAP on rank 0.

The model forward is the HIP path (scda_amd.dropin.models...FasterRCNN_AdEx in eval mode: backbone + RPN + RoIPool + FC on
the MI355X, NMS through scda_nms_hip); this module is only the loop around it.
"""
import json
import logging
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from scda_amd.dropin.utils import bbox_helper
from scda_amd.dropin.utils.cal_mAP import Cal_MAP

logger = logging.getLogger('global')


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def detection_rows(img_id, dts_per_image, gts_per_image, image_info_row, num_classes, resize_scale, coco=False):
    """rows of one image: 100 best by score, then class by class in that order (tools/faster_rcnn_train_val.py:838-858)"""
    rows = []
    order = dts_per_image[:, -2].argsort()[::-1][:100]
    dts_per_image = dts_per_image[order]
    for cls in range(1, num_classes):
        d = dts_per_image[dts_per_image[:, -1] == cls][:, 1:-1]
        d = bbox_helper.clip_bbox(d, image_info_row[:2])
        if len(d) > 0:
            d[:, :4] = d[:, :4] / resize_scale
        for bx in d:
            head = 'val2017/{0}.jpg'.format(img_id) if coco else '{0}'.format(img_id)
            rows.append('{0} {1} {2}\n'.format(head, ' '.join(map(str, bx)), cls))
    return rows


def validate(val_loader, model, cfg, results_dir, val_meta_file=None, dataset='cityscapes', device=None, score=True, batched=False):
    """-> RPN recall (total recalled / total gts).  Loader items: (image [b,3,h,w], image_info [b,>=3], gts [b,G,5], ...,
    filenames).  Distributed when torch.distributed is initialised (each rank writes its own file, rank 0 scores after a
    one-element all-reduce, as the reference synchronises); single-process otherwise (validate_single).
    batched=True: each loader batch goes through scda_amd.infer.predict (the box logic on the device, one host wait per batch)
    instead of the eval-mode forward; the rows written are the same up to the tie rules stated in scda_amd/infer.py."""
    distributed = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if distributed else (0, 1)
    if device is None:
        device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    num_classes = int(cfg['shared']['num_classes'])
    os.makedirs(results_dir, exist_ok=True)
    if rank == 0:   # stale files of a previous, wider run would be concatenated into results.txt
        for f in os.listdir(results_dir):
            if 'results.txt.rank' in f and int(f.split('k')[-1]) >= world:
                logger.info("remove %s" % f)
                os.remove(os.path.join(results_dir, f))
    total_rc = total_gt = 0
    with open(os.path.join(results_dir, 'results.txt.rank%d' % rank), 'w') as fout, torch.no_grad():
        for it, item in enumerate(val_loader):
            img, img_info, gt_boxes, filenames = item[0], item[1], item[2], item[-1]
            t0 = time.time()
            if batched:
                from scda_amd import infer
                proposals, bboxes = infer.rows(*infer.predict(model, img.to(device, non_blocking=True), img_info, cfg))
            else:
                x = {'cfg': cfg, 'image': img.to(device, non_blocking=True), 'image_info': img_info,
                     'ground_truth_bboxes': gt_boxes, 'ignore_regions': None}
                outputs = model(x)['predict']
                proposals, bboxes = _np(outputs[0]), _np(outputs[1])
            t1 = time.time()
            gts_np, info_np = _np(gt_boxes), _np(img_info)
            for b in range(img.shape[0]):
                img_id = filenames[b].rsplit('/', 1)[-1].rsplit('.', 1)[0]
                scale = info_np[b, 2] if dataset == 'coco' else info_np[b, -1]
                rc, ng = bbox_helper.compute_recall(proposals[proposals[:, 0] == b][:, 1:5], gts_np[b])
                total_rc += rc
                total_gt += ng
                fout.writelines(detection_rows(img_id, bboxes[bboxes[:, 0] == b], gts_np[b], info_np[b], num_classes, scale,
                                               coco=(dataset == 'coco')))
                fout.flush()
            logger.info('Test: [%d/%d] Time: %.3f %d/%d' % (it, len(val_loader), t1 - t0, total_rc, total_gt))
    logger.info('rpn300 recall=%f' % (total_rc / total_gt))
    if distributed:
        sync = torch.ones(1, device=device)
        dist.all_reduce(sync)
    if score and rank == 0:
        if dataset == 'coco':
            raise NotImplementedError("COCO scoring needs pycocotools (datasets/pycocotools in the reference); "
                                      "results.txt.rank* are written, score them there")
        Cal_MAP(results_dir, val_meta_file, num_classes)
    if was_training:
        model.train()
    return total_rc / total_gt


def write_segm_results(writer, image_info, image_ids, out, category_of=None, input_resolution=False, keep_num=100):
    """The JSON lines of the reference's write_results_to_file (tools/mask_rcnn_train_val.py:381-430) from one
    scda_amd.infer.Predictor(masks=True, rle=True) pass: per image the `keep_num` best detections by score (ties in the detections'
    order), one line each with `image_id`, `bbox` = [x, y, w, h] of the detection box, `score`, `category_id` (category_of(class), default
    the class index) and `segmentation` = {'size': [h, w], 'counts': str}, the mask's compressed RLE as the device encoded it.
    image_info [B, >=3] rows (h, w, resize_scale, ...); image_ids: B ids.  Returns the number of masks the host had to encode.

    The masks are at the NETWORK-INPUT resolution.  The reference resizes each mask once more to the original image size before it
    thresholds (:422); that resize is not done here, so an image with resize_scale != 1 raises ValueError -- unless the caller passes
    input_resolution=True and then gets box AND mask of such an image at the network-input resolution (the box NOT divided by
    resize_scale, so the two agree) and rescales them himself.

    A pass of Predictor(masks=True, rle=True, original_size=(Ho, Wo)) carries that second resize (its mask_bits_orig): its lines
    are the reference's for any resize_scale -- `bbox` from det_orig (the box divided by resize_scale in float32, :408), `segmentation`
    the RLE of the mask resized to the original size and thresholded there with `>` (:422-423), 'size' = [origin_h, origin_w].
    input_resolution=True has no meaning for such a pass (ValueError); an image beyond the device limits (orig_status) raises ValueError."""
    from scda_amd import infer
    info = _np(image_info)
    if info.ndim != 2 or info.shape[1] < 3 or len(image_ids) != info.shape[0]:
        raise ValueError("write_segm_results: image_info [B, >=3] and B image ids")
    original = getattr(out, 'mask_bits_orig', None) is not None
    if original and input_resolution:
        raise ValueError("write_segm_results: the pass carries original-size results; input_resolution=True does not apply to it")
    if not input_resolution and not original:
        bad = [b for b in range(info.shape[0]) if float(info[b, 2]) != 1.0]
        if bad:
            raise ValueError("write_segm_results: images %s have resize_scale != 1; the masks are encoded at the network-input "
                             "resolution (pass input_resolution=True to get box and mask at that resolution)" % bad)
    segs, fallbacks = infer.segm_rows(out, with_fallbacks=True)
    det, det_counts = _np(out.det_orig if original else out[2]), _np(out[3])
    for b in range(info.shape[0]):
        d = det[b, :int(det_counts[b])]
        order = np.argsort(-d[:, 5], kind='stable')[:keep_num]
        scale = 1.0 if input_resolution or original else float(info[b, 2])
        for ix in order:
            box = (d[ix, 1:5] / np.float32(scale)).tolist()
            cls = int(d[ix, 6])
            seg = segs[b][ix]
            res = {'image_id': int(image_ids[b]), 'bbox': [box[0], box[1], box[2] - box[0], box[3] - box[1]], 'score': d[ix, 5].tolist(),
                   'category_id': category_of(cls) if category_of is not None else cls,
                   'segmentation': {'size': seg['size'], 'counts': seg['counts']}}
            writer.write(json.dumps(res) + '\n')
        writer.flush()
    return fallbacks


def write_keypoint_results(writer, image_info, image_ids, out, category_of=None, keep_num=100):
    """The JSON lines of the reference's write_results_to_file (tools/mask_rcnn_train_val.py:381-430) for the keypoint case (:415-418)
    from one scda_amd.infer.Predictor(keypoints=True) pass: per image the `keep_num` best detections by score (ties in the detections'
    order, as write_segm_results), one line each with `image_id`, `bbox` = [x, y, w, h] of the detection box divided by resize_scale in
    float32 (:408), `score`, `category_id` (category_of(class), default the class index) and `keypoints` = the detection's
    keypoints_orig row flattened to 3 Kp numbers (x, y divided by resize_scale, :417; the third value of each keypoint is the raw
    resized heat-map value).  image_info [B, >=3] rows (h, w, resize_scale, ...); image_ids: B ids.  `out`: the pass's result tuple (its
    last two entries are keypoints, keypoints_orig; an infer.PredictorResult names them)."""
    info = _np(image_info)
    if info.ndim != 2 or info.shape[1] < 3 or len(image_ids) != info.shape[0]:
        raise ValueError("write_keypoint_results: image_info [B, >=3] and B image ids")
    named = getattr(out, 'keypoints_orig', None)
    kps = _np(out[-1] if named is None else named)
    det, det_counts = _np(out[2]), _np(out[3])
    if kps.ndim != 4 or kps.shape[:2] != det.shape[:2] or kps.shape[3] != 3:
        raise ValueError("write_keypoint_results: the pass carries no keypoints (Predictor(keypoints=True))")
    for b in range(info.shape[0]):
        d = det[b, :int(det_counts[b])]
        order = np.argsort(-d[:, 5], kind='stable')[:keep_num]
        for ix in order:
            box = (d[ix, 1:5] / np.float32(info[b, 2])).tolist()
            cls = int(d[ix, 6])
            res = {'image_id': int(image_ids[b]), 'bbox': [box[0], box[1], box[2] - box[0], box[3] - box[1]], 'score': d[ix, 5].tolist(),
                   'category_id': category_of(cls) if category_of is not None else cls,
                   'keypoints': kps[b, ix].reshape(-1).tolist()}
            writer.write(json.dumps(res) + '\n')
        writer.flush()


def coco_stats(loader, predictor, evaluator, device=None, distributed=False, group=None, proposals=False, original_keypoints=False):
    """Drives a scda_amd.infer.Predictor over a loader into a scda_amd.coco_eval.CocoEvaluator and returns COCOeval's 12 stats (numpy
    float64).  Loader items are dicts: 'image' [B, 3, H, W], 'image_info' [B, >= 2], 'image_ids' int32 [B], and the ground truth as
    CocoEvaluator.add takes it -- 'gt_boxes' float64 [B, Gcap, 4] (x, y, w, h), 'gt_areas', 'gt_iscrowd', 'gt_categories', 'gt_counts',
    for 'segm' also 'gt_mask_bits' (infer.pack_masks) and optionally 'sizes' -- IN THE COORDINATES OF THE DETECTIONS (the network input:
    scale the ground truth by resize_scale, nothing is divided here).  Tensors that are on the device already are used as they are; the
    only wait for the host is the last one.  validate() is not involved.

    An item may carry 'annotations' (per image a list of COCO annotation dicts, with 'sizes' = the (h, w) of every image) INSTEAD of
    the six gt_* entries: they are then built by a scda_amd.coco_gt.GroundTruth that is kept across the items -- for 'segm' the masks
    are rasterised on the device (scda_mask_frpoly_hip) into planes of the Predictor's shape, max_gts_per_image slots per image.  The
    annotations are rasterised AT THEIR OWN COORDINATES: as for every other ground-truth input, bringing polygons, boxes and areas to
    the detections' coordinates when resize_scale != 1 is the caller's business.

    A Predictor with original_size=(Ho, Wo) (image_info rows (h, w, resize_scale, origin_h, origin_w)) puts the DETECTIONS at the
    original image's coordinates instead: the evaluator is fed det_orig, mask_bits_orig, the areas of the original-size masks and
    'sizes' = every image's (origin_h, origin_w) -- the item's 'sizes' if it has them, else image_info[:, 3:5] --, and the GroundTruth
    of 'annotations' is built at the planes of mask_bits_orig.  COCO's own annotations then need no rescaling, for 'bbox' and 'segm'
    alike.  The orig_status of every pass is kept on the device and read after the last one: ValueError, in place of stats that empty
    masks would have entered silently, if any image was beyond the device limits (it names the image ids).

    distributed=True, with torch.distributed initialised: the loader is this rank's UNPADDED shard (e.g. Subset(ds, range(rank, n,
    world)); a repeated image id raises ValueError) and CocoEvaluator.merge(group) runs before the summary, so every rank returns the
    same stats.  The orig_status check stays this rank's own.  The default returns this rank's own result.

    proposals=True scores the RPN proposals instead (the reference's test types 'proposal' / 'person_proposal': average recall at 1,
    100 and 1000 proposals with params={'max_dets': [1, 100, 1000]}): the evaluator must be a 'bbox' one built with use_cats=False and
    max_dets_per_image = the Predictor's proposal capacity; it is fed out[0], out[1] through CocoEvaluator.add_proposals in place of
    the detections.  Proposals stand at the network input's coordinates, so a Predictor with original_size is refused here.  A
    use_cats=False evaluator with proposals=False is fed the detections (class rows scored category-agnostically).

    A 'keypoints' evaluator (CocoEvaluator(K, 'keypoints', num_keypoints=Kp)) needs a Predictor(keypoints=True) -- ValueError otherwise
    -- with evaluator.D == the Predictor's top_n and evaluator.Kp == model.num_keypoints.  It is fed the pass's `keypoints` (the network
    input's coordinates, like the detections), or with original_keypoints=True its `keypoints_orig` (x, y divided by resize_scale:
    COCO's own annotations then need no rescaling); the ground truth also carries 'gt_keypoints' float64 [B, Gcap, Kp, 3] and
    'gt_num_keypoints' int32 [B, Gcap], from the item or built from its 'annotations' by coco_gt.flatten_annotations(...,
    keypoints=True).  COCOeval's 10 keypoint stats come back.  proposals=True does not apply."""
    kps = evaluator.iou_type == 'keypoints'
    if kps:
        if not getattr(predictor, 'keypoints', False):
            raise ValueError("coco_stats: a 'keypoints' evaluator needs a Predictor built with keypoints=True (a detector with the "
                             "keypoint branch)")
        if proposals:
            raise ValueError("coco_stats: proposals=True does not apply to a 'keypoints' evaluator")
        top_n, n_kp = int(predictor.box_cfg['top_n']), int(predictor.model.num_keypoints)
        if evaluator.D != top_n or evaluator.Kp != n_kp:
            raise ValueError("coco_stats: the 'keypoints' evaluator holds %d detections of %d keypoints per image, the Predictor gives %d "
                             "of %d" % (evaluator.D, evaluator.Kp, top_n, n_kp))
    elif original_keypoints:
        raise ValueError("coco_stats: original_keypoints=True goes with a 'keypoints' evaluator")
    if proposals and (evaluator.use_cats or evaluator.iou_type != 'bbox'):
        raise ValueError("coco_stats: proposals=True needs a 'bbox' evaluator built with use_cats=False")
    if proposals and getattr(predictor, 'original_size', None) is not None:
        raise ValueError("coco_stats: proposals=True is not covered for a Predictor with original_size")
    segm = evaluator.iou_type == 'segm'
    if segm and not (predictor.masks and predictor.rle):
        raise ValueError("coco_stats: a 'segm' evaluator needs Predictor(masks=True, rle=True)")
    device = evaluator.device if device is None else device
    ground_truth = None
    statuses = []
    with torch.no_grad():
        for item in loader:
            out = predictor(item['image'].to(device, non_blocking=True), item['image_info'])
            original = getattr(predictor, 'original_size', None) is not None
            if original:
                statuses.append((item['image_ids'], out.orig_status.clone()))        # the Predictor's buffer is overwritten by the next pass
            det, bits = (out.det_orig, out.mask_bits_orig) if original else (out[2], out[4] if segm else None)
            sizes = item.get('sizes')
            if original and sizes is None:
                sizes = _np(item['image_info'])[:, 3:5].astype(np.int64)
            if 'annotations' in item:
                from scda_amd import coco_gt, native
                if segm:
                    if ground_truth is None or (ground_truth.H, ground_truth.Wd) != tuple(bits.shape[2:]):
                        ground_truth = coco_gt.GroundTruth(device, evaluator.G, bits.shape[2], bits.shape[3])
                    gt = ground_truth.load(item['annotations'], sizes if original else item['sizes'])
                else:
                    flat = coco_gt.flatten_annotations(item['annotations'], sizes if original else item['sizes'], evaluator.G,
                                                       **({'keypoints': True, 'num_keypoints': evaluator.Kp} if kps else {}))
                    gt = tuple(native.upload(flat[k], device) for k in ('gt_boxes', 'gt_areas', 'gt_iscrowd', 'gt_categories', 'gt_counts'))
                    gt += (None,)
                    if kps:
                        gt_kp = (native.upload(flat['gt_keypoints'], device), native.upload(flat['gt_num_keypoints'], device))
            else:
                gt = (item['gt_boxes'], item['gt_areas'], item['gt_iscrowd'], item['gt_categories'], item['gt_counts'],
                      item['gt_mask_bits'] if segm else None)
                if kps:
                    gt_kp = (item['gt_keypoints'], item['gt_num_keypoints'])
            kw = {}
            if segm:
                kw = {'mask_bits': bits, 'det_areas': out[5]['area'], 'gt_mask_bits': gt[5], 'sizes': sizes}
            if kps:
                kw = {'keypoints': out[-1] if original_keypoints else out[-2], 'gt_keypoints': gt_kp[0], 'gt_num_keypoints': gt_kp[1]}
            if proposals:
                evaluator.add_proposals(item['image_ids'], out[0], out[1], *gt[:5])
            else:
                evaluator.add(item['image_ids'], det, out[3], *gt[:5], **kw)
    _merge_if_distributed(evaluator, distributed, group)
    stats = evaluator.summarize()
    flagged = [(int(i), int(v)) for ids, st in statuses for i, v in zip(_np(ids).reshape(-1), _np(st).reshape(-1)) if v]
    if flagged:
        raise ValueError("coco_stats: images %s (image id, orig_status) are beyond the limits of the original-size masks (see "
                         "infer.Predictor); their masks are empty and the stats would be wrong" % flagged)
    return stats


def meta_ground_truth(val_meta_file, num_classes):
    """The validation meta file (or its lines) as MapEvaluator takes ground truth: {pure_name: int32 [n, 5] = (x1, y1, x2, y2, label), in
    meta order, 'num': int64 [num_classes]}.  The record layout is the one utils.cal_mAP.parse_gts reads: a '#' line, +1 the path (the
    pure name is its last component without the 4-character extension), +7 the box count, +8... `label x1 y1 x2 y2`.  Every row is kept
    as written; rows with a label outside 1..num_classes-1 take no part in the matching and are not counted in 'num'."""
    if isinstance(val_meta_file, (list, tuple)):
        lines = list(val_meta_file)
    else:
        with open(val_meta_file, 'r', encoding='utf-8') as f:
            lines = f.readlines()
    gts = {'num': np.zeros(num_classes, dtype=np.int64)}
    for at, line in enumerate(lines):
        if not line.startswith('#'):
            continue
        name = lines[at + 1].strip().split('/')[-1][0:-4]
        count = int(lines[at + 7])
        rows = np.zeros((count, 5), dtype=np.int32)
        for k, row in enumerate(lines[at + 8: at + 8 + count]):
            f = row.split()
            rows[k] = (int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[0]))
        gts[name] = rows
        labels = rows[:, 4]
        gts['num'] += np.bincount(labels[(labels >= 1) & (labels < num_classes)], minlength=num_classes)[:num_classes]
    return gts


def _merge_if_distributed(evaluator, distributed, group):
    if distributed and dist.is_available() and dist.is_initialized():
        evaluator.merge(group=group)


def map_stats(loader, predictor, evaluator, ground_truth, scale_column=-1, device=None, distributed=False, group=None):
    """Drives a scda_amd.infer.Predictor over validate()'s loader into a scda_amd.map_eval.MapEvaluator and returns its summary: what
    Cal_MAP computes from validate()'s rows (ap, max_recall, mAP) plus validate()'s RPN recall, without the text files and with one
    wait for the host, the last one.  Loader items are validate()'s tuples: item[0] image [b, 3, h, w], item[1] image_info [b, >= 3],
    item[2] gts [b, G, 5] (for the recall, every row counted as the reference counts them), item[-1] filenames.  ground_truth:
    meta_ground_truth(...); each file's pure name is looked up there, an image missing there gets zero ground truths.  scale_column:
    the image_info column the boxes are divided by (-1; 2 is the reference's dataset == 'coco' choice).  validate() is not involved.

    Every image is added with an id: the position of its pure name in the meta file, -1 for an image the meta does not have (such an
    image is never taken for a copy of another).  distributed=True, with torch.distributed initialised: the loader is this rank's
    shard (a DistributedSampler, padding included), and MapEvaluator.merge(group) runs before the summary, so every rank returns the
    SAME dict -- what the reference computes from the concatenated rank files.  The default returns this rank's own result."""
    from scda_amd import native
    device = evaluator.device if device is None else device
    G = evaluator.G
    position = {name: k for k, name in enumerate(n for n in ground_truth if n != 'num')}
    with torch.no_grad():
        for item in loader:
            img, img_info, gt_boxes, filenames = item[0], item[1], item[2], item[-1]
            B = img.shape[0]
            out = predictor(img.to(device, non_blocking=True), img_info)
            on_device = torch.is_tensor(img_info) and img_info.is_cuda and img_info.dtype == torch.float32 and img_info.is_contiguous()
            info = img_info if on_device else predictor.image_info          # the Predictor's own upload of a host image_info
            boxes, counts = np.zeros((B, G, 5), dtype=np.int32), np.zeros(B, dtype=np.int32)
            ids = np.full(B, -1, dtype=np.int32)
            for b in range(B):
                pure = filenames[b].rsplit('/', 1)[-1].rsplit('.', 1)[0]
                rows = ground_truth.get(pure)
                if rows is None or pure == 'num':
                    continue
                ids[b] = position[pure]
                if len(rows) > G:
                    raise ValueError("map_stats: %s has %d ground truths, max_gts_per_image = %d" % (filenames[b], len(rows), G))
                boxes[b, :len(rows)], counts[b] = rows, len(rows)
            evaluator.add(out[2], out[3], info, native.upload(boxes, device), native.upload(counts, device), proposals=out[0],
                          proposal_counts=out[1], recall_gts=native.upload(_np(gt_boxes).astype(np.float32), device),
                          scale_column=scale_column, image_ids=native.upload(ids, device))
    _merge_if_distributed(evaluator, distributed, group)
    return evaluator.summarize()
