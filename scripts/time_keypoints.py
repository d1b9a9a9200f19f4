"""Keypoint inference of the ResNet-50 C4 detector with the keypoint branch at 800 x 1344, B = 2: 100 detections per image from a seeded
untrained detector (boxes drawn as in scripts/time_infer_masks.py), R = 200 RoIs, Kp = 17:
  (i)   the decode alone (scda_keypoint_decode_hip on the Predictor's own RoIs and heat maps), device time between HIP events;
  (ii)  the host predict_keypoints (PIL + numpy) on the same input, one pass, and whether the two agree bit for bit;
  (iii) Predictor ms per batch with and without keypoints=True, eager and replayed as a graph.
Prints one JSON line per configuration and writes them to --out.

    python scripts/time_keypoints.py --out profiles/keypoint_decode_time.txt"""
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
    ap.add_argument("--B", type=int, default=2)
    ap.add_argument("--kp", type=int, default=17)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host pass (a minute of PIL resizes)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scda_amd import infer
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_keypoints
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    dev = torch.device("cuda")
    torch.manual_seed(0)
    det = resnet50(cfg=dict(CFG['shared'], roi_align=True, gan_model_flag=2, with_keypoint=True, num_keypoints=a.kp)).to(dev).eval()
    H, W, B = a.H, a.W, a.B
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(dev)
    info = torch.tensor([[H, W, 1.0]] * B, device=dev)
    lines = []

    def report(**r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def timed(fn, n):
        out = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return [round(1e3 * s / n, 3) for s in out]

    pred = infer.Predictor(det, CFG, keypoints=True)
    out = pred(x, info)
    torch.cuda.synchronize()
    rois, cls, heat = pred.kp_rois.clone(), pred.kp_cls.clone(), pred.keypoint_heat.clone()
    R = rois.shape[0]
    shape = {"H": H, "W": W, "R": R, "Kp": a.kp, "detections": int(out[3].sum()), "heat_contiguous": bool(pred.keypoint_heat.is_contiguous())}
    wh = (rois[:, 3:5] - rois[:, 1:3] + 1).cpu().numpy()
    shape["box_w_mean"], shape["box_h_mean"] = round(float(wh[:, 0].mean()), 1), round(float(wh[:, 1].mean()), 1)
    # (i) the decode alone, on the layout the head returns and on a contiguous copy
    for name, src in (("decode_head_layout", pred.keypoint_heat), ("decode_contiguous", heat.contiguous())):
        res = torch.empty(R, a.kp, 3, device=dev)
        ws = torch.empty(N.keypoint_decode_workspace_bytes(R, a.kp, W), dtype=torch.uint8, device=dev)
        N.keypoint_decode(rois, src, H, W, cls=cls, out=res, ws=ws)
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                N.keypoint_decode(rois, src, H, W, cls=cls, out=res, ws=ws)
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1) / a.iters, 4))
        report(config=name, device_ms_per_call=min(ms), device_ms_all_windows=ms, **shape)
    # (ii) the host rule on the same input
    if not a.no_host:
        r_h, c_h, h_h = rois.cpu().numpy(), cls.cpu().numpy(), heat.cpu().numpy()
        t0 = time.perf_counter()
        want = predict_keypoints(r_h, h_h, np.array([[H, W]] * B), cls=c_h)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(res.cpu().numpy().view(np.uint32), want.view(np.uint32)))
        report(config="host_predict_keypoints", host_ms_per_call=round(1e3 * host_s, 1), equals_device_bit_for_bit=same, **shape)
    # (iii) the Predictor with and without the keypoints
    plain = infer.Predictor(det, CFG)
    plain(x, info)
    for name, p in (("predictor_keypoints", pred), ("predictor_boxes_only", plain)):
        ms = timed(lambda: p(x, info), a.iters)
        report(config=name + "_eager", ms_per_batch=min(ms), ms_per_batch_all_windows=ms, B=B, **shape)
        p.capture(x, info)
        p.replay()
        ms = timed(p.replay, a.iters)
        report(config=name + "_graph", ms_per_batch=min(ms), ms_per_batch_all_windows=ms, B=B, **shape)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/time_keypoints.py on one MI355X, %s; the best of the windows first, every window behind it\n"
                    % torch.cuda.get_device_name(0))
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
