"""Segmentation results at the ORIGINAL image size: the ResNet-50 C4 detector with the mask branch at 800 x 1344, (h, w) = (800, 1067),
original size (480, 640), 100 detections per image from a seeded untrained detector, B = 1 and 4.  Per configuration the pass and the
call that brings the results to the host:
  (i)   Predictor(masks=True, rle=True) + segm_rows                      -- the input-resolution results, as before;
  (ii)  Predictor(masks=True, rle=True, original_size=(480, 640)) + segm_rows  -- the second resize on the device
        (scda_amd/csrc/mask_rescale.hip), the run-length code of the original-size masks;
  (iii) the host route, for its COST: Predictor(masks=True) + mask_rows, then per detection a PIL resize of the boolean mask (already
        thresholded with >= at the input resolution, taken as 0 / 1 floats) to (640, 480), `> 0.5` and scda_amd.mask_rle_host.encode --
        not the masks of (ii), which resizes the pasted float plane.
(i) and (ii) are also timed without segm_rows, ending in a device synchronise.  Every shape is warmed first; each line reports every
timed window and quotes the best.

    python scripts/time_segm_orig.py --out profiles/segm_orig_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_segm_orig.py --quick     # (ii) only: the kernels' times"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.time_infer import CFG  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per configuration")
    ap.add_argument("--host-iters", type=int, default=1, help="passes of the host route per window")
    ap.add_argument("--quick", action="store_true", help="(ii) only, B = 1, 2 iterations, one window (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from PIL import Image
    from scda_amd import infer, mask_rle_host
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    dev = torch.device("cuda")
    torch.manual_seed(0)
    det = resnet50(cfg=dict(CFG['shared'], roi_align=True, gan_model_flag=2, with_mask=True)).to(dev).eval()
    H, W, h, w, oh, ow = 800, 1344, 800, 1067, 480, 640
    iters, repeats = (2, 1) if a.quick else (a.iters, a.repeats)
    g = torch.Generator().manual_seed(1)
    pool = torch.rand(4, 3, H, W, generator=g) * 2 - 1
    lines = []

    def report(name, n_img, windows, **extra):
        best = min(windows)
        r = dict({"config": name, "images_per_window": n_img, "windows": len(windows), "ms_per_image": round(1e3 * best / n_img, 3),
                  "ms_per_image_all_windows": [round(1e3 * s / n_img, 3) for s in windows]}, **extra)
        lines.append(r)
        print(json.dumps(r), flush=True)

    def timed(fn, n):
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return out

    for B in ((1,) if a.quick else (1, 4)):
        x = pool[:B].to(dev)
        info = torch.tensor([[h, w, h / oh, oh, ow]] * B, dtype=torch.float32, device=dev)
        orig = infer.Predictor(det, CFG, masks=True, rle=True, original_size=(oh, ow))
        res = orig(x, info)
        torch.cuda.synchronize()
        n_det = int(res[3].sum())
        assert not res.orig_status.any()
        report("original_size_pass_B%d" % B, B * iters, timed(lambda: orig(x, info), iters), detections=n_det)
        if a.quick:
            continue
        _, fb = infer.segm_rows(res, with_fallbacks=True)
        report("original_size_pass_plus_segm_rows_B%d" % B, B * iters, timed(lambda: infer.segm_rows(orig(x, info)), iters),
               detections=n_det, host_fallbacks=fb)
        del orig
        today = infer.Predictor(det, CFG, masks=True, rle=True)
        infer.segm_rows(today(x, info))
        report("input_resolution_pass_B%d" % B, B * iters, timed(lambda: today(x, info), iters), detections=n_det)
        report("input_resolution_pass_plus_segm_rows_B%d" % B, B * iters, timed(lambda: infer.segm_rows(today(x, info)), iters),
               detections=n_det)
        del today
        masks_only = infer.Predictor(det, CFG, masks=True)

        def host_route():
            out = masks_only(x, info)
            rows = []
            for m in infer.mask_rows(out[4], out[3], w):
                for plane in m[:, :h]:
                    big = np.array(Image.fromarray(plane.astype(np.float32)).resize((ow, oh)))
                    rows.append(mask_rle_host.encode(big > 0.5))
            return rows

        host_route()
        report("host_route_B%d" % B, B * a.host_iters, timed(host_route, a.host_iters), detections=n_det)
        del masks_only
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/time_segm_orig.py on one MI355X, %s; 800 x 1344 input, (h, w) = (800, 1067), original size (480, 640); "
                    "ms_per_image = the best of the windows\n" % torch.cuda.get_device_name(0))
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
