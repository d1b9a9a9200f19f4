"""COCO AP on the device against the numpy statement on a synthetic COCO-val-sized set: 5000 images x 100 detections, 80 categories,
about 7 ground truths per image (detections jittered from the ground truths, scores rounded to two decimals so that ties occur).
  (i)   CocoEvaluator.add per batch of 4 images: device time (HIP events around a pass over all batches), best of the timed windows;
  (ii)  accumulate() + the summarize kernel over all rows: device time, best of the timed windows;
  (iii) tests/coco_eval_np.py -- the same rules as per-image numpy / Python loops, the shape of pycocotools' own evaluator -- wall time
        on this host, measured on the first --np-images images (the loops are linear in the images; the full set takes minutes) and
        stated per image and scaled; the device result on that subset is checked against it bit for bit.
The ratio is reported, not gated: the host number depends on the box.  Prints one JSON line per item and writes them to --out.

    python scripts/time_coco_eval.py --out profiles/coco_eval_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_coco_eval.py --quick       # the kernels' times"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def synthetic(n_images, top_n, K, G, seed=0):
    rs = np.random.RandomState(seed)
    gc = np.clip(rs.poisson(7, n_images), 1, G).astype(np.int32)
    w = np.exp(rs.uniform(np.log(8), np.log(400), (n_images, G))); h = np.exp(rs.uniform(np.log(8), np.log(300), (n_images, G)))
    gb = np.round(np.stack([rs.uniform(0, 1344 - 400, (n_images, G)), rs.uniform(0, 800 - 300, (n_images, G)), w, h], 2), 1)
    live = np.arange(G)[None] < gc[:, None]
    gb[~live] = 0
    gk = np.where(live, rs.randint(1, K + 1, (n_images, G)), 0).astype(np.int32)
    gi = (live & (rs.rand(n_images, G) < 0.1)).astype(np.uint8)
    ga = gb[..., 2] * gb[..., 3]
    pick = (rs.randint(0, 1 << 30, (n_images, top_n)) % gc[:, None])
    src = np.take_along_axis(gb, pick[..., None].repeat(4, 2), 1)
    s = rs.choice([0.03, 0.12, 0.4], (n_images, top_n, 1))
    j = rs.normal(0, 1, (n_images, top_n, 4)) * s
    x1 = src[..., 0] + j[..., 0] * src[..., 2]; y1 = src[..., 1] + j[..., 1] * src[..., 3]
    det = np.zeros((n_images, top_n, 7), np.float32)
    det[..., 1], det[..., 2] = x1, y1
    det[..., 3], det[..., 4] = x1 + src[..., 2] * np.exp(j[..., 2]), y1 + src[..., 3] * np.exp(j[..., 3])
    det[..., 5] = np.round(rs.uniform(0.05, 1.0, (n_images, top_n)), 2)
    cat = np.take_along_axis(gk, pick, 1)
    det[..., 6] = np.where(rs.rand(n_images, top_n) < 0.85, cat, rs.randint(1, K + 1, (n_images, top_n)))
    dc = np.full(n_images, top_n, np.int32)
    ids = rs.permutation(n_images).astype(np.int32) * 7 + 3
    return {'ids': ids, 'det': det, 'dc': dc, 'gb': gb, 'ga': ga, 'gi': gi, 'gk': gk, 'gc': gc}


def np_images(s, n):
    import coco_eval_np as cnp
    out = []
    for i in range(n):
        d, g = int(s['dc'][i]), int(s['gc'][i])
        xywh = cnp.xywh_from_corners(s['det'][i, :d, 1:5])
        out.append({'image_id': int(s['ids'][i]), 'dt_xywh': xywh, 'dt_score': s['det'][i, :d, 5], 'dt_cat': s['det'][i, :d, 6].astype(np.int32),
                    'dt_area': xywh[:, 2] * xywh[:, 3], 'gt_xywh': s['gb'][i, :g], 'gt_area': s['ga'][i, :g], 'gt_iscrowd': s['gi'][i, :g],
                    'gt_cat': s['gk'][i, :g]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--np-images", type=int, default=250)
    ap.add_argument("--quick", action="store_true", help="one pass, no numpy side (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import coco_eval_np as cnp
    from scda_amd import native as N
    from scda_amd.coco_eval import CocoEvaluator
    dev = torch.device("cuda")
    K, top_n, G = 80, 100, 16
    s = synthetic(a.images, top_n, K, G)
    d = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    ev = CocoEvaluator(K, 'bbox', max_images=a.images, max_dets_per_image=top_n, max_gts_per_image=G, device=dev)
    lines = []

    def report(**r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def add_all(n):
        ev.reset()
        for b in range(0, n, a.batch):
            e = min(b + a.batch, n)
            ev.add(d['ids'][b:e], d['det'][b:e], d['dc'][b:e], d['gb'][b:e], d['ga'][b:e], d['gi'][b:e], d['gk'][b:e], d['gc'][b:e])

    def finish():
        ev.accumulate()
        N.coco_summarize(ev.precision, ev.recall, (ev.T, ev.R, ev.K, ev.A, ev.M), ev.d_specs, ev.stats)

    def windows(fn, repeats):
        out = []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            out.append(t0.elapsed_time(t1))
        return out

    repeats = 1 if a.quick else a.repeats
    add_all(a.images); finish(); torch.cuda.synchronize()                     # warm-up
    n_batches = (a.images + a.batch - 1) // a.batch
    w = windows(lambda: add_all(a.images), repeats)
    report(item="add", images=a.images, batch=a.batch, detections_per_image=top_n, categories=K, us_per_batch=round(1e3 * min(w) / n_batches, 2),
           ms_per_pass_all_windows=[round(v, 2) for v in w], note="HIP events around a pass over all batches (launch-bound: includes the host's launch gaps)")
    w = windows(finish, repeats)
    stats = ev.stats.cpu().numpy()
    report(item="accumulate+summarize", rows=a.images * top_n, ms=round(min(w), 3), ms_all_windows=[round(v, 3) for v in w],
           stats=[round(float(v), 6) for v in stats])
    if not a.quick:
        n = min(a.np_images, a.images)
        images = np_images(s, n)
        t0 = time.perf_counter()
        for im in images:
            im['iou'] = cnp.bb_iou(im['dt_xywh'], im['gt_xywh'], im['gt_iscrowd'])
        want = cnp.evaluate(images, K)
        wall = time.perf_counter() - t0
        add_all(n)
        got = {k: v.cpu().numpy() for k, v in ev.accumulate().items()}
        equal = all(np.array_equal(got[k], want[k]) for k in ('precision', 'recall', 'scores'))
        report(item="coco_eval_np", images=n, wall_s=round(wall, 2), ms_per_image=round(1e3 * wall / n, 2),
               scaled_to_all_images_s=round(wall * a.images / n, 1), device_equals_numpy_on_these_images=bool(equal))
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
