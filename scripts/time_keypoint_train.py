"""Training the keypoint branch, timed on one MI355X:
  (i)   the heat-map loss forward + backward at R = 64, Kp = 17, 56 x 56 on the keypoint head's transposed channel-major view
        (scda_amd/csrc/keypoint_loss.hip), against torch.nn.functional.cross_entropy and against autograd_ops.cross_entropy (the
        class-count kernel), each on a contiguous copy of the same tensor on the same device, the copy there and the copy of the gradient
        back included -- device time between HIP events, warm-up first, the median of the windows; each composition eager (where the
        host's 0.1 ms per call hides the kernels) and recorded into a graph and replayed (the launches alone);
  (ii)  ScdaTrainer.step at 800 x 1344 with and without the branch, the two trainers alternating window by window (host clock around
        a window that ends in a synchronise).
Prints one JSON line per configuration and writes them to --out.  Nothing gates on these numbers.

    python scripts/time_keypoint_train.py --out profiles/keypoint_train_time.txt"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--kp", type=int, default=17)
    ap.add_argument("--side", type=int, default=56)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-step", action="store_true", help="skip the trainer iterations")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch.nn.functional as F
    import bench
    from scda_amd import autograd_ops as A
    from scda_amd import resnet_config as RC
    if not torch.cuda.is_available():
        raise SystemExit("time_keypoint_train.py measures on the GPU; no HIP device is visible")
    dev = torch.device("cuda")
    lines = []

    def report(**r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def device_ms(fn):
        for _ in range(5):
            fn()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1) / a.iters, 4))
        return ms

    def graph_ms(fn):
        """fn recorded once into a graph and replayed: the device time of its launches without the host's share (eager, the ~0.1 ms
        of Python and autograd per call are longer than the kernels, and the events measure the host)"""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return device_ms(graph.replay)

    # (i) the loss, forward + backward, on the head's view: [Kp, R, h, w] in memory, seen as [R, Kp, h, w]
    R, Kp, side = a.R, a.kp, a.side
    g = torch.Generator().manual_seed(0)
    base = torch.randn(Kp, R, side, side, generator=g).to(dev).requires_grad_()
    targets = torch.randint(0, side * side, (R, Kp), generator=g, dtype=torch.int32)
    targets[torch.rand(R, Kp, generator=g) < 0.2] = -1                       # one keypoint in five not labelled
    t32, t64 = targets.to(dev), targets.reshape(-1).long().to(dev)
    t64_ignore = torch.where(t64 < 0, torch.full_like(t64, -100), t64)
    shape = {"R": R, "Kp": Kp, "h": side, "w": side, "counted": int((targets >= 0).sum()), "view_bytes": base.numel() * 4}

    def hip_view():
        base.grad = None
        A.keypoint_heatmap_loss(base.transpose(0, 1), t32).backward()

    def torch_copy():
        base.grad = None
        F.cross_entropy(base.transpose(0, 1).contiguous().view(R * Kp, side * side), t64_ignore, ignore_index=-100).backward()

    def class_kernel_copy():
        base.grad = None
        A.cross_entropy(base.transpose(0, 1).contiguous().view(R * Kp, side * side), t64_ignore, -100).backward()

    losses = {}
    for name, fn in (("keypoint_loss_hip_on_view", hip_view), ("torch_cross_entropy_on_copy", torch_copy),
                     ("class_count_kernel_on_copy", class_kernel_copy)):
        fn()
        torch.cuda.synchronize()
        grad = base.grad.clone()
        ms = device_ms(fn)
        losses[name] = grad
        report(config=name + "_eager", device_ms_fwd_bwd=statistics.median(ms), device_ms_all_windows=ms, **shape)
        ms = graph_ms(fn)
        report(config=name + "_graph", device_ms_fwd_bwd=statistics.median(ms), device_ms_all_windows=ms, **shape)
    ref = losses["torch_cross_entropy_on_copy"].double()
    for name in ("keypoint_loss_hip_on_view", "class_count_kernel_on_copy"):
        report(config=name + "_gradient_vs_torch", rel_l2=float((losses[name].double() - ref).norm() / ref.norm()))

    # (ii) the iteration with and without the branch
    if not a.no_step:
        src, tgt, gts, info = bench.synth_batch(0, RC.H, RC.W)
        kps = RC.synth_keypoints(gts, Kp, seed=0)
        src, tgt = src.to(dev), tgt.to(dev)
        runs = {}
        for name, with_kp in (("step_with_keypoint_branch", True), ("step_without_branch", False)):
            torch.manual_seed(0); np.random.seed(0)
            tr = RC.make_trainer(bench.CFG, dev, with_keypoint=with_kp, num_keypoints=Kp)
            run = runs[name] = {"tr": tr, "kw": {"gt_keypoints": kps} if with_kp else {}, "ms": []}
            for _ in range(5):
                run["out"] = tr.step(src, gts, info, tgt, **run["kw"])
        for _ in range(a.repeats):                                           # the two trainers alternate, window by window
            for run in runs.values():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    run["out"] = run["tr"].step(src, gts, info, tgt, **run["kw"])
                torch.cuda.synchronize()
                run["ms"].append(round(1e3 * (time.perf_counter() - t0) / a.steps, 3))
        for name, run in runs.items():
            report(config=name, ms_per_step=statistics.median(run["ms"]), ms_per_step_all_windows=run["ms"], H=RC.H, W=RC.W,
                   keypoint_rois=getattr(run["tr"].model, "last_keypoint_rois", None),
                   keypoint_loss=float(run["out"]["keypoint_loss"]) if run["kw"] else None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/time_keypoint_train.py on one MI355X, %s; the median of the windows first, every window behind it\n"
                    % torch.cuda.get_device_name(0))
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
