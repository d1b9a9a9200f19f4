"""Cluster-region generator: the host path (sklearn k-means + index_select) against the device path (SCDA_DEVICE_KMEANS=1,
scda_amd/device_clusters.py) on one MI355X.  Writes profiles/cluster_device_time.txt (--out).  Reported, not gated.

  calls   per call, host and device path alternated in one process on the 512-RoI sets of tests/golden/kmeans_ref.npz with random
          [512, 4096] features: the calling thread's CPU time and the wall time to a synchronise; warm-up excluded; median and range
  kernels device time of the two kernels from HIP event pairs; the gather as bytes moved over time, next to the HBM bound
  soak    free-running 512 x 1024 iterations with the switch on; at every call the host path also runs on the same RoIs (global RNG
          state saved and restored): calls whose cluster features or crop corners differ, and calls that fell back to the host
  bench   SCDA_DEVICE_KMEANS=0 and =1 under the unchanged `python bench.py --full --no-cpu-baseline`, alternated: images/s and
          host.main_thread_cpu_ms_per_step (with the switch at 0 the step is the parent commit's)

python scripts/time_cluster_targets.py [--parts calls kernels soak bench] [--calls 200] [--soak 300] [--bench-rounds 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_MEASURED_TBS = 6.29      # float4 copy on an MI355X (8.0 TB/s spec)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med_range(v):
    v = np.asarray(v) * 1e3
    return "%.3f ms median (%.3f .. %.3f)" % (np.median(v), v.min(), v.max())


def sets_512():
    g = np.load(os.path.join(ROOT, "tests", "golden", "kmeans_ref.npz"))
    out = []
    for i, name in enumerate(g["names"]):
        p = "s%02d_" % i
        if g[p + "rois"].shape[0] == 512 and int(g[p + "equal"]):
            out.append((str(name), g[p + "rois"], int(g[p + "k"]), int(g[p + "threshold"])))
    return out


def part_calls(dev, n_calls):
    from scda_amd.dropin.functions import mask
    sets = sets_512()
    feats = torch.randn(512, 4096, device=dev)
    rois = []
    for _, r, _, _ in sets:
        t = torch.from_numpy(r).to(dev)
        t._scda_host = r                     # as the trainer hands the sampled RoIs over
        rois.append(t)
    cpu = {"0": [], "1": []}
    wall = {"0": [], "1": []}
    np.random.seed(0)
    for i in range(-20, n_calls):            # 20 warm-up calls per path
        j = i % len(sets)
        for switch in ("0", "1"):
            os.environ["SCDA_DEVICE_KMEANS"] = switch
            torch.cuda.synchronize()
            c0, t0 = time.thread_time(), time.perf_counter()
            mask.compute_cluster_targets(rois[j], feats, N_cluster=sets[j][2], threshold=sets[j][3])
            c1 = time.thread_time()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= 0:
                cpu[switch].append(c1 - c0)
                wall[switch].append(t1 - t0)
    say("calls: %d per path, alternated, %d sets of 512 RoIs (k in {2, 4, 8}), features [512, 4096]" % (n_calls, len(sets)))
    say("  host path    calling thread CPU %s   wall to synchronise %s" % (med_range(cpu["0"]), med_range(wall["0"])))
    say("  device path  calling thread CPU %s   wall to synchronise %s" % (med_range(cpu["1"]), med_range(wall["1"])))
    say("  host CPU per call, device / host: %.3f" % (np.median(cpu["1"]) / np.median(cpu["0"])))


def part_kernels(dev, reps=50):
    from scda_amd import device_clusters, native
    for name, r, k, thr in [s for s in sets_512() if s[0].split("_")[0] in ("uniform", "objects")][::3]:
        n = r.shape[0]
        rois = torch.from_numpy(r).to(dev)
        feats = torch.randn(n, 4096, device=dev)
        first, uniforms, _ = device_clusters.seeding_constants(n, k)
        i32 = dict(dtype=torch.int32, device=dev)
        bufs = {"centres": torch.empty(k, 2, device=dev), "labels": torch.empty(n, **i32), "counts": torch.empty(k, **i32),
                "members": torch.empty(k, n, **i32), "seed_index": torch.empty(k, **i32), "n_iter": torch.empty(1, **i32),
                "status": torch.empty(1, **i32)}
        picks = torch.zeros(k, thr, **i32)
        out = torch.empty(k, thr, 4096, device=dev)
        km, ga = [], []
        for i in range(reps + 5):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            native.kmeans(rois, k, first, uniforms, bufs)
            e[1].record()
            native.cluster_gather(feats, bufs["members"], bufs["counts"], picks, k, thr, out=out)
            e[2].record()
            torch.cuda.synchronize()
            if i >= 5:
                km.append(e[0].elapsed_time(e[1]) * 1e-3)
                ga.append(e[1].elapsed_time(e[2]) * 1e-3)
        moved = 2 * k * thr * 4096 * 4
        say("kernels %-22s k %d n_iter %2d: kmeans %s; gather %s = %.2f TB/s of %d bytes (HBM copy bound %.2f TB/s: %.4f ms)" % (
            name, k, int(bufs["n_iter"].item()), med_range(km), med_range(ga), moved / np.median(ga) * 1e-12, moved, HBM_MEASURED_TBS,
            moved / (HBM_MEASURED_TBS * 1e12) * 1e3))


def part_soak(dev, iters):
    import bench
    from scda_amd import train_step
    from scda_amd.dropin.functions import mask
    from scda_amd.dropin.models.faster_rcnn import faster_rcnn_adver_expansion_reweight_cluster as model
    os.environ["SCDA_DEVICE_KMEANS"] = "1"
    stats = {"calls": 0, "rows": 0, "corners": 0, "host": 0}
    host_path = mask.host_cluster_targets

    def counted(*args, **kw):                # every call of the sklearn path: the comparison's own, and those the device path hands back
        stats["host"] += 1
        return host_path(*args, **kw)

    mask.host_cluster_targets = counted

    def both(rois, features, N_cluster=4, threshold=128):
        state = np.random.get_state()
        want, want_c = mask.host_cluster_targets(rois, features, N_cluster, threshold)
        np.random.set_state(state)
        got, got_c = mask.compute_cluster_targets(rois, features, N_cluster, threshold)
        stats["calls"] += 1
        stats["rows"] += int(not torch.equal(got, want))
        corner = lambda c: train_step.get_corner_from_center(c, 256, bench.W, bench.H)  # noqa: E731
        stats["corners"] += int(corner(got_c) != corner(want_c))
        return got, got_c

    model.compute_cluster_targets = both
    torch.manual_seed(0)
    np.random.seed(100)
    tr = train_step.ScdaTrainer(bench.CFG, dev, lr=1.25e-5, new_w=bench.W, new_h=bench.H)
    for it in range(iters):
        src, tgt, gts, info = bench.synth_batch(it)
        tr.step(src.to(dev), gts, info, tgt.to(dev))
    torch.cuda.synchronize()
    model.compute_cluster_targets = mask.compute_cluster_targets
    mask.host_cluster_targets = host_path
    say("soak: %d free-running %d x %d iterations, switch on: %d calls, %d with different cluster features, %d with different crop "
        "corners, %d fell back to the host path" % (iters, bench.H, bench.W, stats["calls"], stats["rows"], stats["corners"],
                                                    stats["host"] - stats["calls"]))


def part_bench(rounds, steps, warmup):
    """-> False as soon as a bench.py child fails or runs out of time: the caller then starts nothing more on the GPU"""
    res = {"0": [], "1": []}
    for _ in range(rounds):
        for switch in ("0", "1"):
            env = dict(os.environ, SCDA_DEVICE_KMEANS=switch)
            try:
                out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                                      "--full", "--no-cpu-baseline"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
            except subprocess.TimeoutExpired:
                say("bench: SCDA_DEVICE_KMEANS=%s did not finish in 900 s; nothing more is started on the GPU" % switch)
                return False
            if out.returncode != 0:
                say("bench: SCDA_DEVICE_KMEANS=%s exited with %d; nothing more is started on the GPU: %s" % (switch, out.returncode, out.stderr[-400:]))
                return False
            j = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
            res[switch].append((j["value"], j.get("host", {}).get("main_thread_cpu_ms_per_step", float("nan"))))
    for switch in ("0", "1"):
        v = np.array(res[switch])
        say("bench: SCDA_DEVICE_KMEANS=%s  images/s %s (median %.2f)   host.main_thread_cpu_ms_per_step %s (median %.3f)" % (
            switch, " ".join("%.2f" % x for x in v[:, 0]), np.median(v[:, 0]), " ".join("%.3f" % x for x in v[:, 1]), np.median(v[:, 1])))
    return True


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="*", default=["calls", "kernels", "soak", "bench"])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--soak", type=int, default=300)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=40)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_device_time.txt"))
    a = ap.parse_args()
    def write_out():
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    # bench first, before this process opens the GPU: one process on the card at a time.  A child that fails may have faulted the
    # card: what was collected is written and the script ends there, non-zero, without opening the GPU itself.
    if "bench" in a.parts and not part_bench(a.bench_rounds, a.bench_steps, a.bench_warmup):
        write_out()
        sys.exit(1)
    dev = torch.device("cuda:0")
    say("%s, torch %s, sklearn %s, %d host threads visible" % (torch.cuda.get_device_name(0), torch.__version__,
                                                                __import__("sklearn").__version__, os.cpu_count()))
    if "calls" in a.parts:
        part_calls(dev, a.calls)
    if "kernels" in a.parts:
        part_kernels(dev)
    if "soak" in a.parts:
        part_soak(dev, a.soak)
    write_out()
