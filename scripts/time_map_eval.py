"""Cityscapes mAP on the device against the host path on a synthetic validation-sized set: 500 images x 100 detections, 8 classes, about
12 ground truths per image (detections jittered from the ground truths; the scores are not rounded, so that no two rows of an image
share one and the host path's own order among equal scores plays no part).
  (i)   MapEvaluator.add per batch of 4 images: device time (HIP events around a pass over all batches), per timed window;
  (ii)  accumulate() + summarize() over all rows: HIP events, per timed window (the copy of the results to the host included);
  (iii) the host path's evaluation part on the same rows -- evaluate.detection_rows, the text file, utils.cal_mAP.Cal_MAP -- wall time
        on this host over the first --host-images images, stated per image and scaled; the device result on that subset is checked
        against it bit for bit;
  (iv)  --detector: evaluate.validate(batched=True) (score=True) against evaluate.map_stats over the same 64 synthetic 512 x 1024 images
        in batches of 4 with the seeded VGG16 detector of the tests, wall time of the second pass of each.
Nothing is gated: the host numbers depend on the box.  Prints one JSON line per item and writes them to --out.

    python scripts/time_map_eval.py --detector --out profiles/map_eval_time.txt"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def synthetic(n_images, top_n, C, G, seed=0):
    """network-input 512 x 1024 at resize scale 0.5: ground truths in the 1024 x 2048 original"""
    rs = np.random.RandomState(seed)
    gc = np.clip(rs.poisson(12, n_images), 1, G).astype(np.int32)
    w, h = rs.randint(24, 400, (n_images, G)), rs.randint(24, 300, (n_images, G))
    x1, y1 = rs.randint(0, 2048 - 400, (n_images, G)), rs.randint(0, 1024 - 300, (n_images, G))
    gt = np.stack([x1, y1, x1 + w, y1 + h, rs.randint(1, C, (n_images, G))], 2).astype(np.int32)
    pick = rs.randint(0, 1 << 30, (n_images, top_n)) % gc[:, None]
    src = np.take_along_axis(gt, pick[..., None].repeat(5, 2), 1).astype(np.float64)
    size = np.stack([src[..., 2] - src[..., 0], src[..., 3] - src[..., 1]] * 2, 2)
    box = (src[..., :4] + rs.uniform(-1, 1, (n_images, top_n, 4)) * rs.choice([.02, .12, .4], (n_images, top_n, 1)) * size) * .5
    det = np.zeros((n_images, top_n, 7), np.float32)
    det[..., 1:3], det[..., 3:5] = np.minimum(box[..., :2], box[..., 2:]), np.maximum(box[..., :2], box[..., 2:])
    det[..., 5] = rs.uniform(.05, 1.0, (n_images, top_n))
    det[..., 6] = np.where(rs.rand(n_images, top_n) < .85, src[..., 4], rs.randint(1, C, (n_images, top_n)))
    info = np.tile(np.asarray([512, 1024, .5], np.float32), (n_images, 1))
    return {'det': det, 'dc': np.full(n_images, top_n, np.int32), 'info': info, 'gt': gt, 'gc': gc}


def meta_text(names, gts):
    out = []
    for k, (name, g) in enumerate(zip(names, gts)):
        out += ['# %d\n' % k, 'val/city/%s.png\n' % name, '3\n', '1024\n', '2048\n', '0\n', '0\n', '%d\n' % len(g)]
        out += ['%d %d %d %d %d\n' % (r[4], r[0], r[1], r[2], r[3]) for r in g]
    return out


def windows(fn, repeats):
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record(); fn(); t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def detector_part(report, dev, n_images=64, batch=4):
    import seeded_init as si
    from test_host_functions import CFG
    from test_infer_gpu import _detector
    from scda_amd import evaluate, infer
    from scda_amd.map_eval import MapEvaluator
    H, W, G, C = 512, 1024, 12, int(CFG['shared']['num_classes'])
    det = _detector(dev)
    names = ["img%03d_leftImg8bit" % i for i in range(n_images)]
    imgs = [si.synth_images(200 + i, H, W)[0] for i in range(n_images)]
    gts = [si.synth_gts(G, 300 + i, H, W).reshape(1, G, 5).float() for i in range(n_images)]
    loader = [(torch.cat(imgs[b:b + batch]), torch.tensor([[H, W, 1.0]] * batch), torch.cat(gts[b:b + batch]),
               ["leftImg8bit/val/city/%s.png" % n for n in names[b:b + batch]]) for b in range(0, n_images, batch)]
    meta = meta_text(names, [g[0].numpy().astype(np.int32) for g in gts])
    with tempfile.TemporaryDirectory() as tmp:
        meta_file = os.path.join(tmp, "meta.txt")
        with open(meta_file, "w") as f:
            f.writelines(meta)
        gt = evaluate.meta_ground_truth(meta_file, C)
        pred = infer.Predictor(det, CFG)
        ev = MapEvaluator(C, max_images=n_images, max_dets_per_image=int(CFG['test_predict_bbox_cfg']['top_n']), max_gts_per_image=G,
                          device=dev, sum_gt=gt['num'])

        def host():
            try:
                evaluate.validate(loader, det, CFG, os.path.join(tmp, "res"), val_meta_file=meta_file, batched=True)
                return "scored"
            except ValueError as e:                 # a class without rows: the reference's np.max of an empty array
                return "Cal_MAP raised ValueError (%s)" % e

        def device():
            ev.reset()
            return evaluate.map_stats(loader, pred, ev, gt)

        times = {}
        for name, fn in (("validate_batched", host), ("map_stats", device)):
            fn(); torch.cuda.synchronize()          # the first pass packs weights and allocates
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            times[name] = (time.perf_counter() - t0, res)
        report(item="validate(batched=True) vs map_stats", images=n_images, batch=batch, size=[H, W],
               validate_batched_wall_s=round(times["validate_batched"][0], 3), validate_note=times["validate_batched"][1],
               map_stats_wall_s=round(times["map_stats"][0], 3), mAP=float(times["map_stats"][1]['mAP']),
               rpn_recall=float(times["map_stats"][1]['rpn_recall']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-images", type=int, default=125)
    ap.add_argument("--detector", action="store_true", help="also time validate(batched=True) against map_stats with the seeded VGG16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scda_amd import evaluate
    from scda_amd.dropin.utils.cal_mAP import Cal_MAP, cal_mAP, parse_gts, parse_res
    from scda_amd.map_eval import MapEvaluator
    dev = torch.device("cuda")
    C, top_n, G = 9, 100, 32
    s = synthetic(a.images, top_n, C, G)
    d = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
    names = ["img%04d_leftImg8bit" % i for i in range(a.images)]
    gts = [s['gt'][i, :s['gc'][i]] for i in range(a.images)]
    ev = MapEvaluator(C, max_images=a.images, max_dets_per_image=top_n, max_gts_per_image=G, device=dev,
                      sum_gt=evaluate.meta_ground_truth(meta_text(names, gts), C)['num'])
    lines = []

    def report(**r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def add_all(n):
        ev.reset()
        for b in range(0, n, a.batch):
            e = min(b + a.batch, n)
            ev.add(d['det'][b:e], d['dc'][b:e], d['info'][b:e], d['gt'][b:e], d['gc'][b:e])

    def finish():
        ev._accumulated = -1
        return ev.summarize()

    add_all(a.images); finish(); torch.cuda.synchronize()                     # warm-up
    n_batches = (a.images + a.batch - 1) // a.batch
    w = windows(lambda: add_all(a.images), a.repeats)
    report(item="add", images=a.images, batch=a.batch, detections_per_image=top_n, classes=C - 1, us_per_batch=round(1e3 * min(w) / n_batches, 2),
           ms_per_pass_all_windows=[round(v, 2) for v in w], note="HIP events around a pass over all batches (launch-bound: includes the host's launch gaps)")
    w = windows(finish, a.repeats)
    res = finish()
    report(item="accumulate+summarize", rows=a.images * top_n, ms=round(min(w), 3), ms_all_windows=[round(v, 3) for v in w],
           ap=[round(float(v), 6) for v in res['ap']], mAP=float(res['mAP']))
    # ---- the host path's evaluation part on the first n images: detection_rows, the text file, Cal_MAP
    n = min(a.host_images, a.images)
    with tempfile.TemporaryDirectory() as tmp:
        meta_file = os.path.join(tmp, "meta.txt")
        with open(meta_file, "w") as f:
            f.writelines(meta_text(names[:n], gts[:n]))
        t0 = time.perf_counter()
        with open(os.path.join(tmp, "results.txt.rank0"), "w") as f:
            for i in range(n):
                f.writelines(evaluate.detection_rows(names[i], s['det'][i, :s['dc'][i]], None, s['info'][i], C, s['info'][i, -1]))
        with np.errstate(all='ignore'):
            Cal_MAP(tmp, meta_file, C)
        wall = time.perf_counter() - t0
        with open(os.path.join(tmp, "results.txt")) as f, open(meta_file) as g:
            want = cal_mAP(parse_gts(g.readlines(), C), parse_res(f.readlines()), C, 0.5)
    sub = MapEvaluator(C, max_images=n, max_dets_per_image=top_n, max_gts_per_image=G, device=dev,
                       sum_gt=evaluate.meta_ground_truth(meta_text(names[:n], gts[:n]), C)['num'])
    sub.add(d['det'][:n], d['dc'][:n], d['info'][:n], d['gt'][:n], d['gc'][:n])
    got = sub.summarize()
    report(item="host path: detection_rows + text + Cal_MAP", images=n, wall_s=round(wall, 3), ms_per_image=round(1e3 * wall / n, 2),
           scaled_to_all_images_s=round(wall * a.images / n, 2),
           device_equals_host_on_these_images=bool(np.array_equal(got['ap'], want[0]) and np.array_equal(got['max_recall'], want[1])))
    if a.detector:
        detector_part(report, dev)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
