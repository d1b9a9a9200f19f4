"""Generates tests/golden/predict_masks_sweep.npz with the REFERENCE's predict_masks (functions/mask.py:21-49: PIL resize of each
RoI's class plane, pasted into the image), imported UNMODIFIED through tests/golden/ref_harness.py.  Run in the build container:
    python tests/golden/make_golden_predict_masks.py

PIL is present there, so the fixture is entirely the reference's own code (under the Pillow recorded in the file).  24 RoIs on a
96 x 160 plane, 28 x 28 heat maps of 3 classes, two images: 1 x 1, one row, one column, the whole image, boxes touching every border
and corner, fractional coordinates that truncate, sizes around the plane's own 28 (down-scale, identity, up-scale on either axis).
Inputs and outputs only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

H, W = 96, 160
BOXES = [
    (5, 7, 5, 7),                      # 1 x 1
    (10, 20, 60, 20),                  # one row
    (30, 5, 30, 80),                   # one column
    (0, 0, 159, 95),                   # the whole image
    (0, 30, 20, 60), (40, 0, 90, 25), (120, 10, 159, 50), (70, 60, 130, 95),           # left, top, right, bottom border
    (0, 0, 10, 10), (150, 86, 159, 95), (0, 80, 30, 95), (140, 0, 159, 12),           # the four corners
    (12.7, 33.2, 47.9, 70.5), (99.99, 3.01, 131.5, 40.999), (0.9, 0.9, 2.1, 3.999),   # fractions truncate towards zero
    (50, 50, 77, 77),                  # 28 x 28: both passes skipped
    (20, 40, 47, 90), (60, 30, 140, 57),                                              # one pass skipped
    (80, 20, 106, 48), (100, 50, 128, 76),                                            # 27 x 29, 29 x 27
    (33, 44, 45, 56), (70, 10, 71, 49), (90, 70, 129, 71),                            # 13 x 13, 2 x 40, 40 x 2
    (3, 2, 130, 9),                    # wide and flat
]


def case():
    rng = np.random.RandomState(23)
    R = len(BOXES)
    rois = np.zeros((R, 7), dtype=np.float32)
    rois[:, 0] = rng.randint(0, 2, R)
    rois[:, 1:5] = np.array(BOXES, dtype=np.float32)
    rois[:, 5] = rng.rand(R)
    rois[:, 6] = rng.randint(0, 3, R)
    heat = rng.randn(R, 3, 28, 28).astype(np.float32)
    info = np.array([[H, W, 1.0], [H, W, 1.0]], dtype=np.float32)
    return rois, heat, info


def main():
    import PIL
    ns = ref_harness.import_reference()
    rois, heat, info = case()
    pm = ns.mask.predict_masks(torch.from_numpy(rois), torch.from_numpy(heat), info)
    out = np.stack(pm)
    assert out.dtype == np.float32 and out.shape == (len(BOXES), H, W)
    np.savez_compressed(os.path.join(HERE, "predict_masks_sweep.npz"), rois=rois, heatmap=heat, image_info=info, masks=out,
                        pillow=np.array(PIL.__version__))
    print("predict_masks_sweep", out.shape, "Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
