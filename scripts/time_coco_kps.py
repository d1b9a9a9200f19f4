"""Keypoint AP and proposal AR on the device, timed beside the 'bbox' evaluator as it stands (scripts/time_coco_eval.py's synthetic
COCO-val-sized set), HIP events after a warm-up pass, best of the timed windows, all in one session:
  (a) CocoEvaluator.add per batch of 4 images for 'bbox': 100 detection slots, 80 categories, 16 GT slots -- the baseline;
  (b) the same for 'keypoints': 5000 images, 20 detection slots, 8 GT slots, Kp = 17 (scda_coco_kp_rows_hip, scda_coco_oks_hip and
      the match kernel: launch for launch what (a) runs);
  (c) the same for use_cats=False through add_proposals: 1000 proposal slots, 16 GT slots, maxDets [1, 100, 1000] (the rows, box IoU,
      the two regroup kernels and a 1000-wide match);
  (d) accumulate() + the summarize kernel for (b) and (c);
  (e) tests/coco_kps_np.py's wall time per image on a subset, for scale; the device result on that subset is checked against it.
Nothing is gated.  Prints one JSON line per item and writes them to --out.

    python scripts/time_coco_kps.py --out profiles/coco_kps_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_coco_kps.py --quick --images 400      # the kernels' times"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from time_coco_eval import synthetic  # noqa: E402

KP = 17


def synthetic_kps(n_images, D, G, seed=1):
    rs = np.random.RandomState(seed)
    gc = np.clip(rs.poisson(3, n_images), 0, G).astype(np.int32)
    scale = np.exp(rs.uniform(np.log(8), np.log(80), (n_images, G, 1)))
    cx, cy = rs.uniform(100, 900, (n_images, G, 1)), rs.uniform(100, 500, (n_images, G, 1))
    gx = np.round(cx + rs.uniform(-1, 1, (n_images, G, KP)) * scale, 1); gy = np.round(cy + rs.uniform(-1.5, 1.5, (n_images, G, KP)) * scale, 1)
    v = rs.randint(0, 3, (n_images, G, KP)).astype(np.float64) * (rs.rand(n_images, G, 1) >= 0.2)
    gkp = np.stack([gx, gy, v], 3)
    gb = np.stack([gx.min(2), gy.min(2), gx.max(2) - gx.min(2), gy.max(2) - gy.min(2)], 2)
    live = np.arange(G)[None] < gc[:, None]
    ga = gb[..., 2] * gb[..., 3] * rs.choice([0.5, 0.8], (n_images, G))
    gi = (live & (rs.rand(n_images, G) < 0.1)).astype(np.uint8)
    gnk = (v > 0).sum(2).astype(np.int32)
    dc = np.minimum(gc * rs.randint(0, 9, n_images), D).astype(np.int32)
    pick = rs.randint(0, 1 << 30, (n_images, D)) % np.maximum(gc, 1)[:, None]
    src = np.take_along_axis(gkp, pick[:, :, None, None].repeat(KP, 2).repeat(3, 3), 1)
    s = rs.choice([0.03, 0.12, 0.4], (n_images, D, 1, 1)) * np.take_along_axis(scale, pick[:, :, None], 1)[..., None]
    kp = np.ones((n_images, D, KP, 3), np.float32)
    kp[..., :2] = src[..., :2] + rs.normal(0, 1, (n_images, D, KP, 2)) * s
    det = np.zeros((n_images, D, 7), np.float32)
    det[..., 5] = np.round(rs.uniform(0.05, 1.0, (n_images, D)), 2)
    det[..., 6] = 1
    ids = rs.permutation(n_images).astype(np.int32) * 5 + 2
    return {'ids': ids, 'det': det, 'dc': dc, 'kp': kp, 'gkp': gkp, 'gnk': gnk, 'gb': gb, 'ga': ga, 'gi': gi,
            'gk': live.astype(np.int32), 'gc': gc}


def synthetic_props(n_images, P, G, seed=2):
    s = synthetic(n_images, P, 1, G, seed)
    s['prop'] = np.ascontiguousarray(s['det'][..., :6])
    s['prop'][..., 5] = np.round(np.random.RandomState(seed + 1).uniform(0.001, 1.0, (n_images, P)), 3)
    del s['det']
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--np-images", type=int, default=250)
    ap.add_argument("--np-proposal-images", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="one window, no numpy side (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.quick:
        a.repeats = 1
    import coco_eval_np as cnp
    import coco_kps_np as knp
    from scda_amd import native as N
    from scda_amd.coco_eval import CocoEvaluator
    dev = torch.device("cuda")
    lines = []

    def report(**r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def windows(fn):
        out = []
        for _ in range(a.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            out.append(t0.elapsed_time(t1))
        return out

    def finish(ev):
        ev.accumulate()
        N.coco_summarize(ev.precision, ev.recall, (ev.T, ev.R, ev.KE, ev.A, ev.M), ev.d_specs, ev.stats)

    n_batches = (a.images + a.batch - 1) // a.batch
    up = lambda s: {k: torch.from_numpy(v).to(dev) for k, v in s.items()}     # noqa: E731

    def timed(item, ev, add_all, **what):
        add_all(a.images); finish(ev); torch.cuda.synchronize()              # warm-up
        w = windows(lambda: add_all(a.images))
        report(item=item + " add", images=a.images, batch=a.batch, us_per_batch=round(1e3 * min(w) / n_batches, 2),
               ms_per_pass_all_windows=[round(v, 2) for v in w], **what)
        w = windows(lambda: finish(ev))
        report(item=item + " accumulate+summarize", rows=a.images * ev.D, ms=round(min(w), 3), ms_all_windows=[round(v, 3) for v in w],
               stats=[round(float(v), 6) for v in ev.stats.cpu().numpy()])

    # ---- (a) 'bbox' as it stands
    s = synthetic(a.images, 100, 80, 16)
    d = up(s)
    ev = CocoEvaluator(80, 'bbox', max_images=a.images, max_dets_per_image=100, max_gts_per_image=16, device=dev)

    def add_bbox(n, ev=ev, d=d):
        ev.reset()
        for b in range(0, n, a.batch):
            e = min(b + a.batch, n)
            ev.add(d['ids'][b:e], d['det'][b:e], d['dc'][b:e], d['gb'][b:e], d['ga'][b:e], d['gi'][b:e], d['gk'][b:e], d['gc'][b:e])
    timed("(a) bbox", ev, add_bbox, detection_slots=100, categories=80, gt_slots=16)
    del ev, d

    # ---- (b) keypoints
    sk = synthetic_kps(a.images, 20, 8)
    d = up(sk)
    evk = CocoEvaluator(1, 'keypoints', num_keypoints=KP, max_images=a.images, max_dets_per_image=20, max_gts_per_image=8, device=dev)

    def add_kps(n, ev=evk, d=d):
        ev.reset()
        for b in range(0, n, a.batch):
            e = min(b + a.batch, n)
            ev.add(d['ids'][b:e], d['det'][b:e], d['dc'][b:e], d['gb'][b:e], d['ga'][b:e], d['gi'][b:e], d['gk'][b:e], d['gc'][b:e],
                   keypoints=d['kp'][b:e], gt_keypoints=d['gkp'][b:e], gt_num_keypoints=d['gnk'][b:e])
    timed("(b) keypoints", evk, add_kps, detection_slots=20, gt_slots=8, keypoints=KP)
    n = 0 if a.quick else min(a.np_images, a.images)
    params = knp.default_params()
    t0 = time.perf_counter()
    images = []
    for i in range(n):
        nd, ng = int(sk['dc'][i]), int(sk['gc'][i])
        xywh, area = knp.kp_rows(sk['kp'][i, :nd])
        im = {'image_id': int(sk['ids'][i]), 'dt_xywh': xywh, 'dt_area': area, 'dt_score': sk['det'][i, :nd, 5],
              'dt_cat': np.ones(nd, np.int32), 'gt_xywh': sk['gb'][i, :ng], 'gt_area': sk['ga'][i, :ng], 'gt_iscrowd': sk['gi'][i, :ng],
              'gt_cat': np.ones(ng, np.int32), 'gt_ignore': knp.kp_gt_ignore(sk['gi'][i, :ng], sk['gnk'][i, :ng])}
        im['iou'] = knp.oks(sk['kp'][i, :nd], sk['gkp'][i, :ng], im['gt_xywh'], im['gt_area'], params['sigmas'])
        images.append(im)
    if n:
        want = knp.evaluate(images, 1, params, keypoints=True)
        wall = time.perf_counter() - t0
        add_kps(n)
        got = {k: v.cpu().numpy() for k, v in evk.accumulate().items()}
        equal = all(np.array_equal(got[k], want[k]) for k in ('precision', 'recall', 'scores'))
        report(item="(e) coco_kps_np keypoints", images=n, wall_s=round(wall, 2), ms_per_image=round(1e3 * wall / n, 2),
               device_equals_numpy_on_these_images=bool(equal),
               note="equality can fail only where an OKS lies within an ulp of a threshold: the synthetic set has no margin condition")
    del evk, d

    # ---- (c) use_cats=False, proposals
    sp = synthetic_props(a.images, 1000, 16)
    d = up(sp)
    evp = CocoEvaluator(1, 'bbox', max_images=a.images, max_dets_per_image=1000, max_gts_per_image=16, device=dev, use_cats=False,
                        params={'max_dets': [1, 100, 1000]})

    def add_props(n, ev=evp, d=d):
        ev.reset()
        for b in range(0, n, a.batch):
            e = min(b + a.batch, n)
            ev.add_proposals(d['ids'][b:e], d['prop'][b:e], d['dc'][b:e], d['gb'][b:e], d['ga'][b:e], d['gi'][b:e], d['gk'][b:e], d['gc'][b:e])
    timed("(c) use_cats=False proposals", evp, add_props, proposal_slots=1000, gt_slots=16, max_dets=[1, 100, 1000])
    n = 0 if a.quick else min(a.np_proposal_images, a.images)
    pparams = dict(cnp.default_params(), max_dets=[1, 100, 1000])
    t0 = time.perf_counter()
    images = []
    for i in range(n):
        nd, ng = int(sp['dc'][i]), int(sp['gc'][i])
        xywh = cnp.xywh_from_corners(sp['prop'][i, :nd, 1:5])
        images.append({'image_id': int(sp['ids'][i]), 'dt_xywh': xywh, 'dt_area': xywh[:, 2] * xywh[:, 3], 'dt_score': sp['prop'][i, :nd, 5],
                       'dt_cat': np.ones(nd, np.int32), 'gt_xywh': sp['gb'][i, :ng], 'gt_area': sp['ga'][i, :ng],
                       'gt_iscrowd': sp['gi'][i, :ng], 'gt_cat': sp['gk'][i, :ng], 'iou': cnp.bb_iou(xywh, sp['gb'][i, :ng], sp['gi'][i, :ng])})
    if n:
        want = knp.evaluate(images, 1, pparams, use_cats=False)
        wall = time.perf_counter() - t0
        add_props(n)
        got = {k: v.cpu().numpy() for k, v in evp.accumulate().items()}
        equal = all(np.array_equal(got[k], want[k]) for k in ('precision', 'recall', 'scores'))
        report(item="(e) coco_kps_np proposals", images=n, wall_s=round(wall, 2), ms_per_image=round(1e3 * wall / n, 2),
               device_equals_numpy_on_these_images=bool(equal))
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
