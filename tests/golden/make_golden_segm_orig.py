"""Generates tests/golden/segm_orig_ref.npz: the reference's segmentation results at the ORIGINAL image size.  Run in the build
container:
    python tests/golden/make_golden_segm_orig.py [path of the reference checkout]

What runs is the reference's own code and Pillow: predict_masks (functions/mask.py:21-49) imported UNMODIFIED through
tests/golden/ref_harness.py, then lines 422-423 of tools/mask_rcnn_train_val.py as they are spelled there --
    msk = np.array(Image.fromarray(msk).resize((img_w, img_h)));  mask = np.asfortranarray(msk > mask_thresh, dtype=np.uint8)
-- and rleEncode / rleToString of the reference's datasets/pycocotools/common/maskApi.c, compiled unmodified into a temporary directory
as make_golden_mask_rle.py does.  write_results_to_file itself cannot be imported: its module imports models/mask_rcnn/mask_rcnn.py,
which the reference checkout does not have; the two lines above are all it does to a mask before maskUtils.encode.

The cases are the 24 RoIs of make_golden_predict_masks.py on the 96 x 160 plane, with (oh, ow) = (60, 100) 1.6x down, (24, 40) 4x down,
(137, 229) a non-integer up-scale, (96, 160) both passes skipped, (48, 160) and (96, 100) one pass skipped, (1, 1); and one image of
(h, w) = (90, 150) inside the padded 96 x 160 with (oh, ow) = (54, 90).  predict_masks raises for a RoI that leaves its image, so the
last case records the RoIs inside 90 x 150 only (`rois_k` lists them).

The file holds inputs and recorded outputs only: per case k `sizes_k` = (h, w, oh, ow), `rois_k` = the indices of the RoIs recorded,
`orig_k` float32 [n, oh, ow] = line 422's array, `rle_k` = line 423's mask through rleEncode + rleToString at mask_thresh 0.5, the
strings joined by newlines; the RoIs and heat maps (the inputs of predict_masks_sweep.npz, repeated so the file stands alone); the
Pillow version."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402
from make_golden_mask_rle import load_reference, ref_outputs  # noqa: E402
from make_golden_predict_masks import case  # noqa: E402

CASES = (((96, 160), (60, 100)), ((96, 160), (24, 40)), ((96, 160), (137, 229)), ((96, 160), (96, 160)), ((96, 160), (48, 160)),
         ((96, 160), (96, 100)), ((96, 160), (1, 1)), ((90, 150), (54, 90)))
MASK_THRESH = 0.5


def main():
    import PIL
    from PIL import Image
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_harness.REF
    ns = ref_harness.import_reference()
    rois, heat, _ = case()
    out = {'rois': rois, 'heatmap': heat, 'mask_thresh': np.float32(MASK_THRESH), 'pillow': np.array(PIL.__version__)}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_reference(ref_root, tmp)
        for k, ((h, w), (img_h, img_w)) in enumerate(CASES):
            inside = np.array([r for r in range(len(rois)) if int(rois[r, 3]) < w and int(rois[r, 4]) < h])
            info = np.array([[h, w, 1.0, img_h, img_w]] * 2, dtype=np.float32)
            masks = ns.mask.predict_masks(torch.from_numpy(rois[inside]), torch.from_numpy(heat[inside]), info)
            orig, strings = [], []
            for msk in masks:
                msk = np.array(Image.fromarray(msk).resize((img_w, img_h)))
                mask = np.asfortranarray(msk > MASK_THRESH, dtype=np.uint8)
                orig.append(msk)
                strings.append(ref_outputs(lib, mask)[1].tobytes())
            out['sizes_%d' % k] = np.array([h, w, img_h, img_w], dtype=np.int32)
            out['rois_%d' % k] = inside.astype(np.int32)
            out['orig_%d' % k] = np.stack(orig)
            out['rle_%d' % k] = np.frombuffer(b"\n".join(strings), dtype=np.uint8)
            assert out['orig_%d' % k].dtype == np.float32 and out['orig_%d' % k].shape == (len(inside), img_h, img_w)
    path = os.path.join(HERE, "segm_orig_ref.npz")
    np.savez_compressed(path, **out)
    print("segm_orig_ref", len(CASES), "cases, Pillow", PIL.__version__, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
