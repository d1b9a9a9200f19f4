"""COCO segmentation results of the ResNet-50 C4 detector with the mask branch at 800 x 1344, 100 detections per image, B = 1 and 4:
what it costs to get every detection's mask to the host as a run-length string.
  1. predictor_masks_graph_plus_mask_rows   the only route to host-side masks before the device encoder: the packed words are copied
                                            and unpacked on the host (nothing is encoded yet);
  2. ... plus_host_rle                      the same + scda_amd.mask_rle_host.encode per mask (what a user had to do to get RLE);
  3. predictor_masks_rle eager / graph      Predictor(masks=True, rle=True), the results left on the device;
  4. predictor_masks_rle_graph_plus_segm_rows   the same + infer.segm_rows (the strings on the host, overflows encoded there);
  and predictor_masks_graph, the pass without the encoder, for the encoder's own cost.
Two mask contents, because the tree has no trained mask checkpoint and an untrained head gives noise masks with many times the runs of
a real one: `noise` = the seeded untrained detector as it is (the share of masks over the default capacity is printed), `bump` = the same
pass with the mask head's probabilities replaced by a smooth bump per detection (blob masks; that this stands for the run counts of a
trained model is an assumption nobody has measured).  Every shape is warmed up; the configurations of one (B, content) ALTERNATE inside
each of the timed windows' rounds, every window ends in a device synchronise; the best window and all windows are printed.

    python scripts/time_infer_segm.py --out profiles/infer_segm_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_infer_segm.py --quick      # the device configurations only"""
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
    ap.add_argument("--quick", action="store_true", help="device configurations only, 2 iterations, one window (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scda_amd import infer, mask_rle_host
    from scda_amd import native as N
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50

    class ContentPredictor(infer.Predictor):
        """Predictor whose mask probabilities can be replaced (self.bumps [R, h, w]) behind the mask head's pass, which still runs"""
        bumps = None

        def _masks(self, feat, B, H, W):
            N.det_rois(self.det, self.det_counts, self.mask_rois, self.mask_cls)
            logits = self.model.mask_predictor(feat, self.mask_rois).detach()
            R, _, h, w = logits.shape
            if self.mask_planes is None or self.mask_planes.shape != (R, h, w):
                self.mask_planes = torch.empty(R, h, w, dtype=torch.float32, device=logits.device)
            N.mask_select(logits, self.mask_cls, sigmoid=True, out=self.mask_planes)
            if self.bumps is not None:
                self.mask_planes.copy_(self.bumps)
            N.mask_paste(self.mask_rois, self.mask_planes, H, W, cls=self.mask_cls, packed=True, threshold=self.mask_threshold,
                         out=self.mask_bits.view(R, H, -1))
            return self.mask_bits

    dev = torch.device("cuda")
    torch.manual_seed(0)
    det = resnet50(cfg=dict(CFG['shared'], roi_align=True, gan_model_flag=2, with_mask=True)).to(dev).eval()
    H, W = a.H, a.W
    iters, repeats = (2, 1) if a.quick else (a.iters, a.repeats)
    g = torch.Generator().manual_seed(1)
    pool = torch.rand(4, 3, H, W, generator=g) * 2 - 1
    lines = []

    def bump_planes(R, side=28):
        rng = np.random.RandomState(7)
        yy, xx = np.mgrid[:side, :side].astype(np.float32)
        cy, cx = rng.uniform(9, 18, (2, R, 1, 1)).astype(np.float32)
        s = rng.uniform(4, 9, (R, 1, 1)).astype(np.float32)
        return torch.from_numpy(np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)).to(dev)

    def run_alternating(configs, n_img_of):
        """configs: name -> (fn, passes per window); one window of every configuration per round, `repeats` rounds"""
        windows = {k: [] for k in configs}
        for _ in range(repeats):
            for name, (fn, n) in configs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                windows[name].append(time.perf_counter() - t0)
        for name, (fn, n) in configs.items():
            w, n_img = windows[name], n_img_of * n
            r = {"config": name, "H": H, "W": W, "images_per_window": n_img, "windows": len(w),
                 "ms_per_image": round(1e3 * min(w) / n_img, 3), "ms_per_image_all_windows": [round(1e3 * s / n_img, 3) for s in w]}
            lines.append(r)
            print(json.dumps(r), flush=True)

    def host_rle(masks_per_image):
        return [[mask_rle_host.encode(m) for m in masks] for masks in masks_per_image]

    for B in (1, 4):
        x = pool[:B].to(dev)
        info = torch.tensor([[H, W, 1.0]] * B, device=dev)
        for content in ("noise", "bump"):
            pm = ContentPredictor(det, CFG, masks=True)
            pr = ContentPredictor(det, CFG, masks=True, rle=True)
            if content == "bump":
                pm.bumps = pr.bumps = bump_planes(B * int(pr.box_cfg['top_n']))
            out = pr(x, info)
            pm(x, info)
            torch.cuda.synchronize()
            n_runs = out[5]['n_runs'].cpu().numpy()
            real = np.arange(n_runs.shape[1])[None, :] < out[3].cpu().numpy()[:, None]
            rows, n_fb = infer.segm_rows(out, with_fallbacks=True)
            d = out[2].cpu().numpy()[real]                                          # the windows' word columns, as the kernels cut them
            ca, cb = np.maximum(d[:, 1].astype(np.int64), 0), np.minimum(d[:, 3].astype(np.int64) + 2, W)
            window_words = np.maximum((cb + 31) // 32 - ca // 32, 0)
            stats = {"B": B, "content": content, "encoder_read_bytes_per_image_per_pass_hinted": int(window_words.sum()) * H * 4 // B,
                     "encoder_read_bytes_per_image_per_pass_unhinted": int(real.sum()) * H * ((W + 31) // 32) * 4 // B,
                     "detections": int(real.sum()), "capacity_runs": int(pr.rle_cap),
                     "runs_per_mask_mean": round(float(n_runs[real].mean()), 1), "runs_per_mask_max": int(n_runs[real].max()),
                     "masks_over_capacity": int(n_fb), "string_bytes_per_image": round(sum(len(r['counts']) for rr in rows for r in rr) / B),
                     "bytes_to_host_per_image_segm_rows": round((28 * n_runs.size + 12 * B + sum(
                         len(rr) * max([len(r['counts']) for r in rr] + [0]) for rr in rows)) / B) if n_fb == 0 else None,
                     "bytes_to_host_per_image_mask_rows": int(real.sum()) * H * ((W + 31) // 32) * 4 // B}
            lines.append(stats)
            print(json.dumps(stats), flush=True)
            tag = "_%s_B%d" % (content, B)
            configs = {"predictor_masks_rle_eager" + tag: (lambda: pr(x, info), iters)}
            run_alternating(configs, B)                                            # eager first: capture fixes the buffers afterwards
            pm.capture(x, info); pm.replay()
            pr.capture(x, info); pr.replay()
            torch.cuda.synchronize()
            slow = 1 if content == "noise" and n_fb else iters
            configs = {"predictor_masks_graph" + tag: (pm.replay, iters), "predictor_masks_rle_graph" + tag: (pr.replay, iters)}
            if not a.quick:
                configs["predictor_masks_graph_plus_mask_rows" + tag] = (lambda: infer.mask_rows(pm.replay()[4], pm.det_counts), iters)
                configs["predictor_masks_rle_graph_plus_segm_rows" + tag] = (lambda: infer.segm_rows(pr.replay()), slow)
                configs["predictor_masks_graph_plus_mask_rows_plus_host_rle" + tag] = (
                    lambda: host_rle(infer.mask_rows(pm.replay()[4], pm.det_counts)), 1)
                for fn, _ in list(configs.values())[2:]:
                    fn()                                                           # warm-up of the host sides
            run_alternating(configs, B)
            del pm, pr
    if a.out:
        with open(a.out, "w") as f:
            f.write("# scripts/time_infer_segm.py on one MI355X, %s; ms_per_image = the best of the windows; the configurations of one "
                    "(B, content) alternate inside every round\n" % torch.cuda.get_device_name(0))
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
