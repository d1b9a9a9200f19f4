"""Times the test-time box prediction (native.box_predict: decode + sort, per-class NMS, per-image top_n) with the hard NMS and with
each soft-NMS method, and the host-loop path for the same head outputs (download + compute_predicted_bboxes around the Python loop
of cython_nms.soft_nms -- what soft-NMS cost before the kernel), at the evaluation shape: B in {1, 8}, P = 300, C = 9.

    python scripts/time_soft_nms.py [--out profiles/soft_nms_time.txt] [--runs 25]

Device times: HIP events around one call, after warm-up, the median of --runs.  Host-loop times: wall clock, the median of
--host-runs (B = 8: --host-runs-b8; a run is 64 lists of 300 rows through a Python double loop)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scda_amd import native as N  # noqa: E402
from scda_amd.dropin import backend  # noqa: E402

STDS, MEANS = [0.1, 0.1, 0.2, 0.2], [0, 0, 0, 0]
H, W, TOP_N = 512, 1024, 100
SETTINGS = (("hard NMS (nms_iou_thresh 0.5)", None),
            ("soft, method hard", {'method': 'hard'}), ("soft, method linear", {'method': 'linear'}),
            ("soft, method gaussian", {'method': 'gaussian'}))


def synth_head(B, P, C, seed=0):
    """RoIs in clusters of 8 (a class list overlaps a lot, like a detector's), soft-maxed scores, deltas ~ N(0, 0.5)"""
    rs = np.random.RandomState(seed)
    rois = np.zeros((B * P, 5), dtype=np.float32)
    for b in range(B):
        k = (P + 7) // 8
        x1, y1 = rs.uniform(0, W - 200, k), rs.uniform(0, H - 150, k)
        base = np.stack([x1, y1, x1 + rs.uniform(30, 190, k), y1 + rs.uniform(24, 140, k)], 1)
        box = np.repeat(base, 8, 0)[:P] + rs.uniform(-8, 8, (P, 4))
        box[:, 0::2] = np.clip(box[:, 0::2], 0, W - 1); box[:, 1::2] = np.clip(box[:, 1::2], 0, H - 1)
        box[:, 2:] = np.maximum(box[:, 2:], box[:, :2])
        rois[b * P:(b + 1) * P, 0] = b
        rois[b * P:(b + 1) * P, 1:] = box[rs.permutation(P)]
    logits = rs.randn(B * P, C) * 2
    e = np.exp(logits - logits.max(1, keepdims=True))
    prob = (e / e.sum(1, keepdims=True)).astype(np.float32)
    loc = (rs.randn(B * P, 4 * C) * 0.5).astype(np.float32)
    return rois, prob, loc, np.array([[H, W, 1.0]] * B, dtype=np.float32)


def device_ms(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--host-runs-b8", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P, C = 300, 9
    lines = ["# scripts/time_soft_nms.py on one MI355X: box_predict at P = %d, C = %d, top_n = %d, score_thresh 0 (every class list holds" % (P, C, TOP_N),
             "# all %d rows), RoIs in clusters of 8.  device: HIP events, median (min) of %d runs after 5 warm-up calls, ms" % (P, a.runs),
             "# host loop: the head outputs downloaded + compute_predicted_bboxes around the Python loop of cython_nms.soft_nms, wall clock, ms",
             "%-3s %-30s %12s %10s %10s %16s %6s" % ("B", "NMS", "device median", "device min", "detections", "host loop median", "runs")]
    for B in (1, 8):
        rois, prob, loc, info = synth_head(B, P, C)
        t = [torch.from_numpy(x).to(dev) for x in (rois, prob, loc, info)]
        counts = torch.full((B,), P, dtype=torch.int32, device=dev)
        det, dc = torch.zeros(B, TOP_N, 7, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        ws = torch.empty(N.box_predict_workspace_bytes(B, P, C), dtype=torch.uint8, device=dev)
        for label, soft in SETTINGS:
            setting = N.soft_nms_setting(soft)
            fn = lambda: N.box_predict(t[0], counts, t[1], t[2], t[3], STDS, MEANS, 0.0, 0.5, TOP_N, ws, det, dc, soft_nms=setting)  # noqa: E731
            med, lo = device_ms(fn, a.runs)
            n_det = int(dc.sum().item())
            host, runs = "", ""
            if soft is not None:
                from scda_amd.dropin.functions.predict_bbox import compute_predicted_bboxes
                cfg = {'bbox_normalize_stats_precomputed': True, 'bbox_normalize_stds': STDS, 'bbox_normalize_means': MEANS,
                       'score_thresh': 0.0, 'nms_iou_thresh': 0.5, 'top_n': TOP_N, 'soft_nms': soft}
                backend.use(nms=lambda d, th: None)                    # a substituted hook: the soft path runs the host loop per list
                try:
                    runs = a.host_runs if B == 1 else a.host_runs_b8
                    w = []
                    for _ in range(runs):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rows = compute_predicted_bboxes(t[0].cpu(), t[1].cpu(), t[2].cpu(), t[3].cpu(), cfg)
                        w.append((time.perf_counter() - t0) * 1e3)
                    assert rows.shape[0] == n_det, (rows.shape, n_det)
                    host = "%.1f" % statistics.median(w)
                finally:
                    backend.reset()
            lines.append("%-3d %-30s %12.3f %10.3f %10d %16s %6s" % (B, label, med, lo, n_det, host, runs))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
