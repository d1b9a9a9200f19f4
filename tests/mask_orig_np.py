"""A numpy statement of the rule of scda_mask_rescale_hip (include/scda_ops.h): the reference's write_results_to_file
(tools/mask_rcnn_train_val.py:422-423) on top of predict_masks -- the pasted float plane of a detection, its top-left h x w image
resized by Pillow to the original (oh, ow), `> threshold`, the bit packing, the footprint outside which nothing is set, and the limits
the device flags.  The resize and the paste are the statements of tests/test_mask_infer_rules.py, reused by import.
tests/test_mask_orig_rules.py pins this file to PIL.Image.resize and to tests/golden/segm_orig_ref.npz; the GPU tests compare the kernel
with it."""
import numpy as np

from test_mask_infer_rules import paste_statement, resize_plane

MAX_RATIO = 4            # scda_mask_rescale_max_ratio()
FLAG_CAPACITY, FLAG_EMPTY, FLAG_RATIO, FLAG_INPUT = 1, 2, 4, 8


def sub_plane(roi, plane, H, W, h, w, cls=None):
    """P [h, w]: the paste of one RoI into the padded [H, W] plane, its top-left h x w image"""
    c = None if cls is None else np.array([cls])
    return np.ascontiguousarray(paste_statement(roi[None], plane[None], H, W, c)[0, :h, :w])


def resize_statement(P, oh, ow):
    """O [oh, ow] = P as Pillow resizes a mode-F image (horizontal pass first, a pass of equal sizes skipped)"""
    return resize_plane(P, ow, oh)


def tap_range(n_in, n_out, xx):
    """the taps [xmin, xmax) of output sample xx of an axis n_in -> n_out (equal sizes: the sample itself)"""
    if n_in == n_out:
        return xx, xx + 1
    scale = n_in / n_out
    support = 2.0 * max(scale, 1.0)
    center = (xx + 0.5) * scale
    return max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n_in)


def window(roi, h, w, cls=None):
    """the paste's window of a RoI clipped to the h x w image: (xa, xb, ya, yb), or None for an empty mask"""
    if cls is not None and cls < 0:
        return None
    if not np.all(np.abs(roi[1:5]) < 5e8):
        return None
    x1, y1, x2, y2 = (int(v) for v in roi[1:5])
    if x2 - x1 + 1 <= 0 or y2 - y1 + 1 <= 0:
        return None
    xa, xb, ya, yb = max(x1, 0), min(x2 + 1, w), max(y1, 0), min(y2 + 1, h)
    return (xa, xb, ya, yb) if xa < xb and ya < yb else None


def footprint(roi, h, w, oh, ow, cls=None):
    """(fx1, fy1, fx2, fy2), inclusive: the output samples with a tap inside the window on both axes; (0, 0, -1, -1) when there are none"""
    win = window(roi, h, w, cls)
    if win is None:
        return (0, 0, -1, -1)
    xa, xb, ya, yb = win
    xs = [x for x in range(ow) if (lambda lo, hi: lo < hi and hi > xa and lo < xb)(*tap_range(w, ow, x))]
    ys = [y for y in range(oh) if (lambda lo, hi: lo < hi and hi > ya and lo < yb)(*tap_range(h, oh, y))]
    if not xs or not ys:
        return (0, 0, -1, -1)
    assert xs == list(range(xs[0], xs[-1] + 1)) and ys == list(range(ys[0], ys[-1] + 1))
    return (xs[0], ys[0], xs[-1], ys[-1])


def status_of(info_row, H, W, Ho, Wo):
    """the flag of one image_info row (h, w, scale, oh, ow)"""
    v = np.asarray(info_row, dtype=np.float32)[[0, 1, 3, 4]]
    if not np.all(np.abs(v) < 5e8):
        return FLAG_INPUT
    h, w, oh, ow = (int(x) for x in v)
    flag = 0
    if oh > Ho or ow > Wo:
        flag |= FLAG_CAPACITY
    if oh < 1 or ow < 1:
        flag |= FLAG_EMPTY
    if h < 1 or w < 1 or h > H or w > W:
        flag |= FLAG_INPUT
    if h > MAX_RATIO * oh or w > MAX_RATIO * ow:
        flag |= FLAG_RATIO
    return flag


def statement(rois, planes, H, W, image_info, masks_per_image, Ho, Wo, cls=None, flag_limits=True):
    """rois [R, >= 5], planes [R, ph, pw], image_info [B, >= 5] -> (O float32 [R, Ho, Wo], zero outside each image's oh x ow,
    foot int [R, 5], status int32 [B]).  flag_limits=False: the rule itself for images the device would flag for their ratio."""
    R = rois.shape[0]
    B = (R + masks_per_image - 1) // masks_per_image
    out = np.zeros((R, Ho, Wo), dtype=np.float32)
    foot = np.zeros((R, 5), dtype=np.int64)
    status = np.array([status_of(image_info[b], H, W, Ho, Wo) for b in range(B)], dtype=np.int32)
    if not flag_limits:
        status &= ~FLAG_RATIO
    for r in range(R):
        b = r // masks_per_image
        foot[r] = (b, 0, 0, -1, -1)
        if status[b]:
            continue
        h, w, oh, ow = (int(image_info[b][k]) for k in (0, 1, 3, 4))
        c = None if cls is None else int(cls[r])
        foot[r, 1:] = footprint(rois[r], h, w, oh, ow, c)
        out[r, :oh, :ow] = resize_statement(sub_plane(rois[r], planes[r], H, W, h, w, c), oh, ow)
    return out, foot, status


def pack_gt(values, threshold, sizes):
    """float [R, Ho, Wo] + per plane (oh, ow) -> uint32 [R, Ho, ceil(Wo/32)]: bit (c % 32) of word c // 32 = (value > threshold) inside
    oh x ow, zero outside"""
    R, Ho, Wo = values.shape
    Wd = (Wo + 31) // 32
    bits = np.zeros((R, Ho, Wd * 32), dtype=np.uint64)
    for r in range(R):
        oh, ow = sizes[r]
        bits[r, :oh, :ow] = values[r, :oh, :ow] > threshold
    return (bits.reshape(R, Ho, Wd, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
