"""Ground-truth masks of one image of 64 annotations at 800 x 1344 (planes [800, 42]), two ways to get them onto the device:
  (1) from the annotations: coco_gt.flatten_annotations on the host, the upload of the flat arrays and scda_mask_frpoly_hip
      (GroundTruth.load) -- host wall time of the whole call until the device has finished, the device time of upload + kernels (HIP
      events around load) and of the kernels alone (events around native.mask_frpoly on arrays that are already there);
  (2) from dense masks, which is what the evaluator needed before: infer.pack_masks of bool [64, 800, 1344] on the host and the upload of
      the packed planes -- host wall time until the device has them.  (Building the dense masks on the host, pycocotools' annToMask, is
      NOT in (2): the dense masks are taken as given.)
The annotations are synthetic: 1..3 jittered ellipses of 16..96 vertices each, every eighth one a crowd given as an uncompressed RLE.
Warm-up first, then --repeats windows of each; the best and all windows are reported, with the bytes that cross to the device.  The
planes of (1) are checked against those of (2) once.  Prints one JSON line per item and writes them to --out.

    python scripts/time_gt_masks.py --out profiles/gt_masks_time.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, G = 800, 1344, 64


def synthetic_annotations(seed=0):
    rs = np.random.RandomState(seed)
    anns = []
    for g in range(G):
        cx, cy = rs.uniform(100, W - 100), rs.uniform(80, H - 80)
        rx, ry = np.exp(rs.uniform(np.log(10), np.log(350))), np.exp(rs.uniform(np.log(10), np.log(250)))
        polys = []
        for _ in range(rs.randint(1, 4)):
            k = rs.randint(16, 97)
            a = np.sort(rs.uniform(0, 2 * np.pi, k))
            r = rs.uniform(0.8, 1.1, k)
            ox, oy = rs.uniform(-rx, rx) * 0.6, rs.uniform(-ry, ry) * 0.6
            xy = np.stack([cx + ox + rx * r * np.cos(a), cy + oy + ry * r * np.sin(a)], 1)
            polys.append(np.round(np.clip(xy, [0, 0], [W, H]), 2).reshape(-1).tolist())
        anns.append({'segmentation': polys, 'bbox': [cx - rx, cy - ry, 2 * rx, 2 * ry], 'area': float(np.pi * rx * ry), 'iscrowd': 0,
                     'category_id': 1 + g % 80})
    return anns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scda_amd import coco_gt, infer, native as N
    dev = torch.device("cuda")
    Wd = W // 32
    anns = synthetic_annotations()
    gt = coco_gt.GroundTruth(dev, G, H, Wd)
    bits = gt.load([anns], (H, W))[5]
    torch.cuda.synchronize()
    words = bits.cpu().numpy().reshape(G, H, Wd)
    dense = np.unpackbits(words.view(np.uint8), axis=-1, bitorder='little').reshape(G, H, W).astype(bool)
    # every eighth annotation as a crowd: the uncompressed RLE of its own mask (rleEncode's column-major runs)
    for g in range(0, G, 8):
        t = dense[g].T.reshape(-1).astype(np.int8)
        bounds = np.concatenate([[0], np.flatnonzero(np.diff(np.concatenate([[0], t]))), [t.size]])
        anns[g] = dict(anns[g], segmentation={'size': [H, W], 'counts': np.diff(bounds).tolist()}, iscrowd=1)
    lines = []

    def report(**r):
        lines.append(r)
        print(json.dumps(r), flush=True)

    def timed(fn, repeats):
        """-> (host wall ms until the device is idle, device ms between the events) per window"""
        wall, devt = [], []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s = time.perf_counter()
            t0.record(); fn(); t1.record()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - s)); devt.append(t0.elapsed_time(t1))
        return wall, devt

    r3 = lambda v: [round(x, 3) for x in v]                                   # noqa: E731
    # (1) annotations -> flat arrays -> upload -> kernels
    load = lambda: gt.load([anns], (H, W))                                    # noqa: E731
    for _ in range(3):
        load()
    wall, devt = timed(load, a.repeats)
    flat = coco_gt.flatten_annotations([anns], (H, W), G, plane=(H, Wd))
    s = time.perf_counter()
    for _ in range(a.repeats):
        coco_gt.flatten_annotations([anns], (H, W), G, plane=(H, Wd))
    flatten_ms = 1e3 * (time.perf_counter() - s) / a.repeats
    d = {k: N.upload(v.view(np.int32) if v.dtype == np.uint32 else v, dev) for k, v in flat.items()}
    area = torch.empty(G, dtype=torch.int32, device=dev)
    kern = lambda: N.mask_frpoly(d['xy'], d['poly_first'], d['poly_plane'], d['rle_counts'], d['rle_first'], d['rle_plane'], d['sizes'],   # noqa: E731
                                 gt._ws, gt._bits, area=area)
    for _ in range(3):
        kern()
    _, kdev = timed(kern, a.repeats)
    flat_bytes = int(sum(v.nbytes for v in flat.values()))
    report(item="annotations", annotations=G, polygons=int(len(flat['poly_plane'])), vertices=int(len(flat['xy'])), rles=int(len(flat['rle_plane'])),
           run_counts=int(len(flat['rle_counts'])), bytes_to_device=flat_bytes, host_wall_ms=round(min(wall), 3), host_wall_ms_all=r3(wall),
           of_which_flatten_ms=round(flatten_ms, 3), device_ms_upload_and_kernels=round(min(devt), 3), device_ms_kernels=round(min(kdev), 3),
           device_ms_kernels_all=r3(kdev), workspace_bytes=int(gt._ws.numel()))
    # (2) dense masks -> pack_masks -> upload
    got = gt.load([anns], (H, W))[5].cpu().numpy().reshape(G, H, Wd)
    packed = infer.pack_masks(dense)
    equal = bool(np.array_equal(packed.numpy(), got))
    dense_path = lambda: N.upload(infer.pack_masks(dense), dev)               # noqa: E731
    for _ in range(2):
        dense_path()
    wall2, _ = timed(dense_path, a.repeats)
    up = lambda: N.upload(packed, dev)                                        # noqa: E731
    wall3, dev3 = timed(up, a.repeats)
    report(item="dense_masks", masks=G, dense_bytes_on_host=int(dense.nbytes), bytes_to_device=int(packed.numel() * 4),
           host_wall_ms=round(min(wall2), 3), host_wall_ms_all=r3(wall2), of_which_upload_wall_ms=round(min(wall3), 3),
           device_ms_upload=round(min(dev3), 3), planes_equal_those_from_annotations=equal)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    if not equal:
        sys.exit("the planes from the annotations differ from pack_masks of the dense masks")


if __name__ == "__main__":
    main()
