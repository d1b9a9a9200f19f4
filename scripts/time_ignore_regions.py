"""compute_anchor_targets / compute_proposal_targets with ignore regions on one MI355X: per call the calling thread's CPU time, the wall
time to a synchronise, and the bytes copied host -> device and device -> host.  Reported, not gated.

It calls only the two dropin functions (scda_amd/dropin/functions), so it runs unchanged on a checkout that predates the device path
for ignore regions (there both calls fall back to numpy: the IoU matrix, the target maps and the candidates cross PCIe) -- run it in
both checkouts, alternated, with the same --out; every run appends one block under its --tag.

Inputs: feature size (1, 60, 32, 64) (30720 anchors), 12 gts, 8 ignore regions (one of them a padded zero row), 2000 proposals, all
device tensors; the gts carry their host copy, as the detector's forward attaches it.  Bytes are counted in a pass of their own,
at the tensor API (Tensor.to / .cpu / .cuda / .copy_ between a host and a device tensor), not in the timed calls.

python scripts/time_ignore_regions.py [--tag NAME] [--calls 100] [--out profiles/ignore_regions_time.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHARED = {"anchor_scales": [2, 4, 8, 16, 32], "anchor_ratios": [0.5, 1, 2], "anchor_stride": 16,
          "bbox_normalize_stats_precomputed": True, "bbox_normalize_stds": [0.1, 0.1, 0.2, 0.2],
          "bbox_normalize_means": [0, 0, 0, 0], "num_classes": 9}
ANCHOR_CFG = dict(SHARED, rpn_batch_size=256, nms_iou_thresh=0.7, positive_iou_thresh=0.7, negative_iou_thresh=0.3,
                  positive_percent=0.5, ignore_iou_thresh=0.5)
PROPOSAL_CFG = dict(SHARED, batch_size=512, positive_iou_thresh=0.5, negative_iou_thresh_hi=0.5, negative_iou_thresh_lo=0.0,
                    ignore_iou_thresh=0.5, positive_percent=0.25, append_gts=True)
FS, H, W, G, I, N_PROP = (1, 60, 32, 64), 512, 1024, 12, 8, 2000


def inputs(dev):
    rs = np.random.RandomState(3)

    def boxes(n, lo, hi):
        w, h = rs.uniform(lo, hi, n), rs.uniform(lo, hi / 2, n)
        x, y = rs.uniform(0, 1, n) * (W - 1 - w), rs.uniform(0, 1, n) * (H - 1 - h)
        return np.stack([x, y, x + w, y + h], 1)
    gts = np.hstack([boxes(G, 30, 300), rs.randint(1, 9, (G, 1))]).astype(np.float32)[None]
    ign = boxes(I, 80, 400).astype(np.float32)[None]
    ign[0, -1] = 0
    props = np.hstack([np.zeros((N_PROP, 1)), boxes(N_PROP, 10, 250), np.sort(rs.uniform(0, 1, (N_PROP, 1)), 0)[::-1]]).astype(np.float32)
    gts_dev = torch.from_numpy(gts).to(dev)
    gts_dev._scda_host = gts
    return gts_dev, torch.from_numpy(ign).to(dev), torch.from_numpy(props), torch.tensor([[H, W, 1.0]])


class CopyCounter:
    """bytes that cross between a host and a device tensor at the tensor API while installed"""

    def __init__(self):
        self.h2d = self.d2h = 0
        self.saved = {}

    def _count(self, src, dst):
        if torch.is_tensor(src) and torch.is_tensor(dst) and src.is_cuda != dst.is_cuda:
            n = dst.numel() * dst.element_size()
            if dst.is_cuda:
                self.h2d += n
            else:
                self.d2h += n

    def __enter__(self):
        T = torch.Tensor
        for name in ("to", "cpu", "cuda", "copy_"):
            self.saved[name] = getattr(T, name)
        counter, saved = self, self.saved

        def to(t, *a, **k):
            out = saved["to"](t, *a, **k)
            counter._count(t, out)
            return out

        def cpu(t, *a, **k):
            out = saved["cpu"](t, *a, **k)
            counter._count(t, out)
            return out

        def cuda(t, *a, **k):
            out = saved["cuda"](t, *a, **k)
            counter._count(t, out)
            return out

        def copy_(t, src, *a, **k):
            counter._count(src, t)
            return saved["copy_"](t, src, *a, **k)
        T.to, T.cpu, T.cuda, T.copy_ = to, cpu, cuda, copy_
        return self

    def __exit__(self, *exc):
        for name, f in self.saved.items():
            setattr(torch.Tensor, name, f)


def med_range(v):
    v = np.asarray(v) * 1e3
    return "%.3f ms median (%.3f .. %.3f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="this checkout")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ignore_regions_time.txt"))
    a = ap.parse_args()
    from scda_amd.dropin.functions.anchor_target import compute_anchor_targets
    from scda_amd.dropin.functions.proposal_target import compute_proposal_targets
    dev = torch.device("cuda:0")
    gts, ign, props, info = inputs(dev)
    fns = {"anchor targets  ": lambda r: compute_anchor_targets(FS, ANCHOR_CFG, gts, info, r),
           "proposal targets": lambda r: compute_proposal_targets(props, PROPOSAL_CFG, gts, info, r)}
    lines = ["[%s] %s, torch %s: %s, G %d, I %d, %d proposals, device inputs, %d calls each after 10 warm-up calls" % (
        a.tag, torch.cuda.get_device_name(0), torch.__version__, FS, G, I, N_PROP, a.calls)]
    np.random.seed(0)
    for name, fn in fns.items():
        for what, regions in (("ignore regions", ign), ("none", None)):
            cpu, wall = [], []
            for i in range(-10, a.calls):
                torch.cuda.synchronize()
                c0, t0 = time.thread_time(), time.perf_counter()
                fn(regions)
                c1 = time.thread_time()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= 0:
                    cpu.append(c1 - c0)
                    wall.append(t1 - t0)
            with CopyCounter() as cc:
                fn(regions)
                torch.cuda.synchronize()
            lines.append("  %s  %-14s  calling thread CPU %s   wall to synchronise %s   copied host->device %d B, device->host %d B" % (
                name, what, med_range(cpu), med_range(wall), cc.h2d, cc.d2h))
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
