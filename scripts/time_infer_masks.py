"""Instance-mask inference of the ResNet-50 C4 detector with the mask branch at 800 x 1344, 100 detections per image from a seeded
untrained detector, B = 1 and 4:
  (i)  host route -- the only one before Predictor(masks=True): infer.predict + infer.rows + mask_predictor on the rows + the sigmoid +
       the host predict_masks (one PIL resize and one full-image float plane per detection) + >= 0.5;
  (ii) Predictor(masks=True), eager and replayed as a graph, ending in a device synchronise (the packed masks stay on the device), and
       the same followed by infer.mask_rows (the copy of the words and the unpacking on the host).
Prints one JSON line per configuration and writes them to --out.

    python scripts/time_infer_masks.py --out profiles/infer_masks_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_infer_masks.py --quick     # (ii) only: the kernels' times"""
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
    ap.add_argument("--H", type=int, default=800)
    ap.add_argument("--W", type=int, default=1344)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per configuration (each line reports every window)")
    ap.add_argument("--host-iters", type=int, default=2, help="passes of the host route per window")
    ap.add_argument("--quick", action="store_true", help="(ii) only, 2 iterations, one window (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scda_amd import infer
    from scda_amd.dropin.functions.mask import predict_masks
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    dev = torch.device("cuda")
    torch.manual_seed(0)
    det = resnet50(cfg=dict(CFG['shared'], roi_align=True, gan_model_flag=2, with_mask=True)).to(dev).eval()
    H, W = a.H, a.W
    iters, repeats = (2, 1) if a.quick else (a.iters, a.repeats)
    g = torch.Generator().manual_seed(1)
    pool = torch.rand(4, 3, H, W, generator=g) * 2 - 1
    lines = []

    def report(name, n_img, windows, **extra):
        best = min(windows)
        r = dict({"config": name, "H": H, "W": W, "images_per_window": n_img, "windows": len(windows),
                  "ms_per_image": round(1e3 * best / n_img, 3), "ms_per_image_all_windows": [round(1e3 * s / n_img, 3) for s in windows],
                  "images_per_s": round(n_img / best, 2)}, **extra)
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

    def host_route(x, info):
        res = infer.predict(det, x, info, CFG)
        _, dets = infer.rows(*res)
        with torch.no_grad():
            feat = det.feature_extractor(x)
            logits = det.mask_predictor(feat, torch.from_numpy(dets[:, :5].copy()).to(dev))
            prob = torch.sigmoid(logits)
        planes = predict_masks(dets, prob, info)
        return [p >= 0.5 for p in planes]

    for B in (1, 4):
        x = pool[:B].to(dev)
        info = torch.tensor([[H, W, 1.0]] * B, device=dev)
        pred = infer.Predictor(det, CFG, masks=True)
        out = pred(x, info)
        torch.cuda.synchronize()
        n_det = int(out[3].sum())
        if not a.quick:
            host_route(x, info)                                                   # warm-up of its own shapes
            report("host_route_B%d" % B, B * a.host_iters, timed(lambda: host_route(x, info), a.host_iters), detections=n_det)
        report("predictor_masks_eager_B%d" % B, B * iters, timed(lambda: pred(x, info), iters), detections=n_det)
        pred.capture(x, info)
        pred.replay()
        report("predictor_masks_graph_B%d" % B, B * iters, timed(pred.replay, iters), detections=n_det)
        if not a.quick:
            report("predictor_masks_graph_plus_mask_rows_B%d" % B, B * iters,
                   timed(lambda: infer.mask_rows(pred.replay()[4], pred.det_counts), iters), detections=n_det)
            plain = infer.Predictor(det, CFG)
            plain(x, info)
            report("predictor_boxes_only_eager_B%d" % B, B * iters, timed(lambda: plain(x, info), iters), detections=n_det)
            del plain
        del pred
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/time_infer_masks.py on one MI355X, %s; ms_per_image = the best of the windows\n" % torch.cuda.get_device_name(0))
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
