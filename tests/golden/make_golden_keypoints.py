"""Generates tests/golden/keypoints_ref.npz: the keypoint decode rule (include/scda_ops.h: scda_keypoint_decode_hip) computed by the
REFERENCE's predict_masks (functions/mask.py:21-49), imported UNMODIFIED through tests/golden/ref_harness.py, followed by numpy's
argmax.  Run in the build container:
    python tests/golden/make_golden_keypoints.py

The reference has no heat-map -> keypoint code of its own (its models/mask_rcnn/mask_rcnn.py is missing); the rule is this project's
choice and THIS is what it is pinned to: predict_masks is called once per keypoint k with the class column set to k, each result is
cropped to its RoI's window and given to np.argmax; the row is (x1 + px, y1 + py, the value there).

Two groups, inputs rebuilt by `sweep_case()` / `extra_case()` (the 24 x 3 random 56 x 56 planes would not fit a committed file):
  sweep   the 24 boxes of make_golden_predict_masks.py on the 96 x 160 plane (1 x 1, one row, one column, the whole 160-wide image --
          which crosses a 128-column strip of the kernel --, borders, corners, truncating fractions, skipped passes, down-scales),
          Kp = 3 random-normal 56 x 56 planes per box;
  extra   on a 128 x 200 plane, three planes for every box: (a) a constant plane -- every resized value is equal (asserted here under
          the Pillow that runs this), so the answer is (x1, y1): any reduction that does not honour row-major order across lanes and
          strips fails it; (b) three equal peaks at [10, 40], [30, 5], [30, 6]; (c) an all-negative plane (the maximum must not be a
          zero from outside the window).  Boxes: 56 x 56 (both passes skipped: the identity, tie -> first), 112 x 112, 90 x 70, 56 wide
          and 61 tall / 101 wide and 56 tall (one pass skipped), a down-scale, the whole image.
Outputs, boxes and the Pillow version only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from make_golden_predict_masks import BOXES, H, W  # noqa: E402

KP = 3
PLANE = 56
EXTRA_H, EXTRA_W = 128, 200
EXTRA_BOXES = [
    (20, 10, 75, 65),                  # 56 x 56: both passes skipped
    (5, 3, 116, 114),                  # 112 x 112
    (100, 40, 189, 109),               # 90 x 70
    (30, 60, 85, 120), (60, 2, 160, 57),                                              # one pass skipped
    (150, 100, 170, 110),              # a down-scale on both axes
    (0, 0, 199, 127),                  # the whole image: two strips
]
PEAKS = [(10, 40), (30, 5), (30, 6)]


def sweep_case():
    rng = np.random.RandomState(29)
    R = len(BOXES)
    rois = np.zeros((R, 7), dtype=np.float32)
    rois[:, 0] = rng.randint(0, 2, R)
    rois[:, 1:5] = np.array(BOXES, dtype=np.float32)
    rois[:, 5] = rng.rand(R)
    heat = rng.randn(R, KP, PLANE, PLANE).astype(np.float32)
    info = np.array([[H, W, 1.0], [H, W, 1.0]], dtype=np.float32)
    return rois, heat, info


def extra_case():
    rng = np.random.RandomState(31)
    R = len(EXTRA_BOXES)
    rois = np.zeros((R, 7), dtype=np.float32)
    rois[:, 1:5] = np.array(EXTRA_BOXES, dtype=np.float32)
    planes = np.zeros((3, PLANE, PLANE), dtype=np.float32)
    planes[0] = np.float32(0.37)
    planes[1] = rng.rand(PLANE, PLANE).astype(np.float32) * np.float32(0.5)
    for y, x in PEAKS:
        planes[1, y, x] = np.float32(3.0)
    planes[2] = -(np.float32(1.0) + rng.rand(PLANE, PLANE).astype(np.float32))
    heat = np.ascontiguousarray(np.broadcast_to(planes, (R,) + planes.shape))
    info = np.array([[EXTRA_H, EXTRA_W, 1.0]], dtype=np.float32)
    return rois, heat, info


def decode_with(predict_masks, rois, heat, info):
    """the rule through the reference's function: one call per keypoint, the class column = k"""
    R, Kp = heat.shape[:2]
    out = np.zeros((R, Kp, 3), dtype=np.float32)
    for k in range(Kp):
        rows = rois.copy()
        rows[:, 6] = k
        images = predict_masks(torch.from_numpy(rows), torch.from_numpy(heat), info)
        for r in range(R):
            x1, y1, x2, y2 = (int(v) for v in rows[r, 1:5])
            window = images[r][y1:y2 + 1, x1:x2 + 1]
            assert window.shape == (y2 - y1 + 1, x2 - x1 + 1) and window.dtype == np.float32
            py, px = np.unravel_index(np.argmax(window), window.shape)
            out[r, k] = (x1 + px, y1 + py, window[py, px])
    return out


def main():
    import PIL
    import ref_harness
    ns = ref_harness.import_reference()
    rois, heat, info = sweep_case()
    sweep = decode_with(ns.mask.predict_masks, rois, heat, info)
    erois, eheat, einfo = extra_case()
    extra = decode_with(ns.mask.predict_masks, erois, eheat, einfo)
    # (a): every resized value of the constant plane equals the constant, so the first pixel of the window wins
    for r, (x1, y1, x2, y2) in enumerate(EXTRA_BOXES):
        full = ns.mask.predict_masks(torch.from_numpy(erois[r:r + 1]), torch.from_numpy(eheat[r:r + 1]), einfo)[0]
        assert (full[y1:y2 + 1, x1:x2 + 1] == eheat[r, 0, 0, 0]).all(), "the constant plane does not stay constant under this Pillow"
        assert tuple(extra[r, 0]) == (x1, y1, eheat[r, 0, 0, 0])
    assert tuple(extra[0, 1]) == (20 + 40, 10 + 10, 3.0)                       # the identity: the first of the three equal peaks
    assert (extra[:, 2, 2] < 0).all()
    np.savez_compressed(os.path.join(HERE, "keypoints_ref.npz"), sweep_boxes=rois[:, :5], sweep=sweep, extra_boxes=erois[:, :5],
                        extra=extra, pillow=np.array(PIL.__version__))
    print("keypoints_ref", sweep.shape, extra.shape, "Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
