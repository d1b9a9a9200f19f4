"""Generates tests/golden/ignore_regions_ref.npz: the REFERENCE's compute_anchor_targets (functions/anchor_target.py:16-116) and
compute_proposal_targets (functions/proposal_target.py:17-177), imported UNMODIFIED through tests/golden/ref_harness.py, called with
ignore regions on the cases of tests/ignore_region_cases.py.  Run in the build container:
    python tests/golden/make_golden_ignore_regions.py

Per case, float32 inputs as tensors and np.random.seed(case seed) before the call; stored under '<case name>/': the inputs, every
output, and the full np.random.get_state() the call left behind.  Each case also runs with ignore_regions=None: the regions must
change at least one output (a case that does not test them is a mistake in the case), except the cases marked no_effect, where
outputs AND generator state must be the same.  The `expect` entries of a case are asserted on the reference's output here, with the
reference's own IoU / IoF helpers, so that a case is known to sit on the rule its name states."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import ignore_region_cases as IC  # noqa: E402
import ref_harness  # noqa: E402

OUT = os.path.join(HERE, "ignore_regions_ref.npz")


def rng_entries():
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    assert kind == "MT19937"
    return {"rng_keys": keys, "rng_pos": np.int64(pos), "rng_has_gauss": np.int64(has_gauss), "rng_gauss": np.float64(gauss)}


def run_anchor(ref, c, ign):
    np.random.seed(c["seed"])
    cls_t, loc_t, loc_m, norm = ref.anchor_target.compute_anchor_targets(
        c["fs"], c["cfg"], torch.from_numpy(c["gts"]), torch.from_numpy(c["info"]), None if ign is None else torch.from_numpy(ign))
    assert cls_t.dtype == torch.int64 and loc_t.dtype == torch.float32 and loc_m.dtype == torch.float32
    out = {"cls_targets": cls_t.numpy().astype(np.int8), "loc_targets": loc_t.numpy(), "loc_masks": loc_m.numpy(),
           "normalizer": np.int64(norm)}
    out.update(rng_entries())
    return out


def run_proposal(ref, c, ign):
    np.random.seed(c["seed"])
    rois, labels, t, w = ref.proposal_target.compute_proposal_targets(
        torch.from_numpy(c["props"]), c["cfg"], torch.from_numpy(c["gts"]), torch.from_numpy(c["info"]),
        None if ign is None else torch.from_numpy(ign))
    assert rois.dtype == torch.float32 and labels.dtype == torch.int64 and t.dtype == torch.float32 and w.dtype == torch.float32
    out = {"rois": rois.numpy(), "labels": labels.numpy().astype(np.int16), "loc_targets": t.numpy(), "loc_weights": w.numpy()}
    out.update(rng_entries())
    return out


def same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a))


def flat_labels(cls_targets, fs):          # [1,A,fh,fw] -> [KA] in anchor order
    return cls_targets.reshape(fs[1] // 4, fs[2], fs[3]).transpose(1, 2, 0).reshape(-1)


def has_row(rois, row):
    return bool((rois[:, 1:5] == np.array(row, dtype=np.float32)[None]).all(axis=1).any())


def check_anchor(ref, c, out, plain):
    e, fs, cfg = c["expect"], c["fs"], c["cfg"]
    lab = flat_labels(out["cls_targets"], fs)
    anchors = IC.grid(fs)
    np.testing.assert_array_equal(anchors, ref.anchor_helper.get_anchors_over_plane(fs[2], fs[3], cfg["anchor_ratios"], cfg["anchor_scales"],
                                                                                  cfg["anchor_stride"]))
    iou = ref.bbox_helper.bbox_iou_overlaps(anchors, c["gts"][0])
    iof = ref.bbox_helper.bbox_iof_overlaps(anchors, c["ign"][0]).max(axis=1)
    assert iof.dtype == np.float64
    inside = iof > cfg["ignore_iou_thresh"]
    if "anchor" in e:
        at = iof[e["anchor"]]
        assert (at == cfg["ignore_iou_thresh"] if e["label"] == 0 else at > cfg["ignore_iou_thresh"]) and lab[e["anchor"]] == e["label"], c["name"]
        assert flat_labels(plain["cls_targets"], fs)[e["anchor"]] == 0
    if e.get("fg_by_iou_inside"):
        best_per_gt = iou.max(axis=0)
        best_per_gt[best_per_gt < 0.1] = -1          # (:61) the padded row claims no anchor
        not_argmax = ~(iou == best_per_gt[None]).any(axis=1)
        assert ((lab == 1) & inside & not_argmax & (iou.max(axis=1) > cfg["positive_iou_thresh"])).sum() >= 2, c["name"]
    if e.get("fg_by_argmax_inside"):
        assert not (iou.max(axis=1) > cfg["positive_iou_thresh"]).any()
        assert ((lab == 1) & inside).sum() >= 1 and (lab == 1).sum() == ((lab == 1) & inside).sum(), c["name"]
    if e.get("no_background"):
        assert inside.all() and not (lab == 0).any() and (lab == 1).any() and int(out["normalizer"]) == int((lab == 1).sum()), c["name"]
    if e.get("both_draws"):
        budget = cfg["rpn_batch_size"]
        assert (lab == 1).sum() == int(cfg["positive_percent"] * budget) and (lab == 0).sum() == budget - (lab == 1).sum(), c["name"]
        assert (flat_labels(plain["cls_targets"], fs) == 1).sum() == (lab == 1).sum()


def check_proposal(ref, c, out, plain):
    e, cfg = c["expect"], c["cfg"]
    gts = c["gts"][0]
    gts = gts[(gts[:, 2] > gts[:, 0] + 1) & (gts[:, 3] > gts[:, 1] + 1)]
    cand = ref.bbox_helper.clip_bbox(np.vstack([c["props"][:, 1:5], gts[:, :4]]), c["info"][0])
    assert cand.dtype == np.float32
    ign = c["ign"][0]
    ign = ign[ign[:, 2] - ign[:, 0] > 1]
    if ign.shape[0] == 0:
        assert c["no_effect"]
        return
    iof = ref.bbox_helper.bbox_iof_overlaps(cand, ign).max(axis=1)
    assert iof.dtype == np.float32
    inside = iof > cfg["ignore_iou_thresh"]
    if "n_ignored" in e:
        assert inside.sum() == e["n_ignored"], (c["name"], inside.sum())
    if "min_ignored" in e:
        assert inside.sum() >= e["min_ignored"], (c["name"], inside.sum())
    for row in e.get("present", ()):
        assert has_row(out["rois"], row) and has_row(plain["rois"], row), c["name"]
    for row in e.get("absent", ()):
        assert not has_row(out["rois"], row) and has_row(plain["rois"], row), c["name"]
    if e.get("no_background"):
        assert (out["labels"] > 0).all() and (plain["labels"] == 0).any(), c["name"]
    if e.get("fg_inside"):
        fg_rows = out["rois"][out["labels"] > 0][:, 1:5]
        fg_iof = ref.bbox_helper.bbox_iof_overlaps(fg_rows, ign).max(axis=1)
        plain_fg = plain["rois"][plain["labels"] > 0][:, 1:5]       # (the padding may repeat rows: compare the distinct ones)
        assert (fg_iof > cfg["ignore_iou_thresh"]).sum() >= 2 and np.array_equal(np.unique(fg_rows, axis=0), np.unique(plain_fg, axis=0)), c["name"]
    if "differs_at_thresh" in e:
        other = run_proposal(ref, dict(c, cfg=dict(cfg, ignore_iou_thresh=e["differs_at_thresh"])), c["ign"])
        assert not same(out, other, ("rois", "labels")), c["name"]


def main():
    ref = ref_harness.import_reference()
    store, by_name = {}, {}
    for c in IC.all_cases():
        run, check = (run_anchor, check_anchor) if c["kind"] == "anchor" else (run_proposal, check_proposal)
        out, plain = run(ref, c, c["ign"]), run(ref, c, None)
        outputs = [k for k in out if not k.startswith("rng_")]
        if c["no_effect"]:
            assert same(out, plain), c["name"] + ": marked no_effect, but the ignore regions changed the result or the generator state"
        else:
            assert not same(out, plain, outputs), c["name"] + ": the ignore regions change nothing"
        check(ref, c, out, plain)
        by_name[c["name"]] = out
        if "differs_from" in c["expect"]:
            assert not same(out, by_name[c["expect"]["differs_from"]], outputs), c["name"]
        n = c["name"]
        for k in ("gts", "ign", "info", "props"):
            if k in c:
                store[f"{n}/{k}"] = c[k]
        for k, v in out.items():
            store[f"{n}/{k}"] = v
        print("%-32s I=%-3d %s" % (n, c["ign"].shape[1], {k: (int(v) if np.ndim(v) == 0 else v.shape) for k, v in out.items() if k != "rng_keys"}))
    np.savez_compressed(OUT, **store)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
