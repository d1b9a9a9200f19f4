"""Ignore regions on the device paths (scda_amd/device_boxes.py; box_ops.hip: scda_anchor_label_ign_hip, scda_proposal_match_ign_hip):

  * every case of tests/ignore_region_cases.py through the two dropin functions with DEVICE tensors, bit-equal to what the
    reference's own functions produced (tests/golden/ignore_regions_ref.npz), generator state included, with the numpy IoF made
    to raise -- a silent fall-back to the host fails;
  * one ScdaTrainer.step with ignore regions, device path against the numpy path (SCDA_DEVICE_BOXES=0; pinned to the reference by
    tests/test_ignore_regions.py): every logged loss and one sha256 over all parameters and Adam moments bit-identical, and a
    step without the regions differs;
  * the entry points without ignore regions against the new ones with I = 0."""
import hashlib
import os

import numpy as np
import pytest
import torch

import ignore_region_cases as IC
import model_common as mc
from test_ignore_regions import assert_case_equals_golden, run_case

pytestmark = pytest.mark.gpu

CASES = IC.all_cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ignore_regions_ref.npz"))


@pytest.fixture()
def no_numpy_iof(monkeypatch):
    from scda_amd.dropin.utils import bbox_helper

    def raiser(*a, **k):
        raise AssertionError("bbox_iof_overlaps on the host: the call left the device path")
    monkeypatch.setattr(bbox_helper, "bbox_iof_overlaps", raiser)


@pytest.mark.parametrize("where", ["device", "host_rows"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_path_equals_reference(cuda, golden, no_numpy_iof, case, where):
    """device: gts and ignore regions are plain device tensors.  host_rows: the gts carry their host copy (as the detector's forward
    attaches it) and the ignore regions stay a host tensor (as the loader yields them) -- the upload on the side stream"""
    def place(a):
        t = torch.from_numpy(a)
        if a.shape[-1] == 4 and where == "host_rows":
            return t
        d = t.to(cuda)
        if where == "host_rows":
            d._scda_host = a
        return d
    out = run_case(case, golden, place)
    assert_case_equals_golden(case, golden, out)


def _l2_inputs(golden_dir, cuda):
    g = np.load(os.path.join(golden_dir, "l2_G12.npz"))
    return torch.from_numpy(g["gts"][0]).to(cuda).contiguous(), torch.from_numpy(g["proposals"]).to(cuda).contiguous(), g["image_info"]


def _sentinel(bufs):
    for k, t in bufs.items():
        if torch.is_tensor(t) and t.is_cuda:
            t.view(torch.uint8).fill_(0x5a)
    return bufs


def test_old_entry_points_equal_new_ones_without_rows(cuda, golden_dir):
    """scda_anchor_label_hip / scda_proposal_match_hip against scda_anchor_label_ign_hip / scda_proposal_match_ign_hip with I = 0 on
    the l2_G12 inputs: every output buffer in full (pre-filled, so that what a call leaves untouched compares too)"""
    from scda_amd import device_boxes as DB, native as N
    from test_host_functions import CFG
    gts, props, info = _l2_inputs(golden_dir, cuda)
    cfg = CFG["train_anchor_target_cfg"]
    a32, a64 = DB.anchors_on_device(32, 64, cfg, cuda)
    KA, i32 = a32.shape[0], dict(dtype=torch.int32, device=cuda)

    def anchor_bufs():
        return _sentinel({"best_iou": torch.empty(KA, dtype=torch.float32, device=cuda), "best_gt": torch.empty(KA, **i32),
                          "gt_best": torch.empty(64, **i32), "labels": torch.empty(KA, dtype=torch.int8, device=cuda),
                          "pos_list": torch.empty(KA, **i32), "neg_list": torch.empty(KA, **i32), "counts": torch.empty(2, **i32)})
    old, new = anchor_bufs(), anchor_bufs()
    N.anchor_label(a32, gts, cfg["negative_iou_thresh"], cfg["positive_iou_thresh"], 0.1, old)
    N.anchor_label_ign(a32, gts, cfg["negative_iou_thresh"], cfg["positive_iou_thresh"], 0.1, None, None, 0.5, new)
    torch.cuda.synchronize()
    assert int(old["counts"][0]) > 0 and int(old["counts"][1]) > 0
    for k in old:
        assert torch.equal(old[k].view(torch.uint8), new[k].view(torch.uint8)), k

    pcfg = CFG["train_proposal_target_cfg"]
    n = props.shape[0] + gts.shape[0]

    def match_bufs():
        return _sentinel({"rois": torch.empty(n, 4, dtype=torch.float32, device=cuda), "best_iou": torch.empty(n, dtype=torch.float32, device=cuda),
                          "best_gt": torch.empty(n, **i32), "labels": torch.empty(n, dtype=torch.int8, device=cuda),
                          "pos_list": torch.empty(n, **i32), "neg_list": torch.empty(n, **i32), "counts": torch.empty(2, **i32)})
    old, new = match_bufs(), match_bufs()
    args = (props, gts, float(info[0][0]), float(info[0][1]), pcfg["positive_iou_thresh"], pcfg["negative_iou_thresh_hi"],
            pcfg["negative_iou_thresh_lo"])
    N.proposal_match(*args, old)
    N.proposal_match_ign(*args, None, 0.5, new)
    torch.cuda.synchronize()
    assert int(old["counts"][0]) > 0 and int(old["counts"][1]) > 0
    for k in old:
        assert torch.equal(old[k].view(torch.uint8), new[k].view(torch.uint8)), k


LOSSES = ('rpn_cls', 'rpn_loc', 'rcnn_cls', 'rcnn_loc', 'adloss', 'dis_patch_loss', 'recon_loss', 'fake_loss1_source',
          'fake_loss_target', 'fake_loss_source', 'loss')


def _state_hash(tr):
    h = hashlib.sha256()
    for k in sorted(tr.flat):
        for t in (tr.flat[k].data, tr.opt[k].exp_avg, tr.opt[k].exp_avg_sq):
            h.update(t.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_trainer_step_with_ignore_regions(cuda, monkeypatch):
    """256 x 512, the small configuration of tests/model_common.py: the step whose box logic runs on the device equals, bit for bit,
    the step whose box logic runs in numpy; the regions bite (a step without them logs other losses)"""
    from scda_amd.train_step import ScdaTrainer
    from test_train_step_gpu import build_product
    H, W = 256, 512
    ign = torch.tensor([[[0, 0, 260, 255], [300, 100, 511, 255], [0, 0, 0, 0]]], dtype=torch.float32)

    def one_step(device_boxes, regions, want_hash=True):
        monkeypatch.setenv("SCDA_DEVICE_BOXES", "1" if device_boxes else "0")
        torch.manual_seed(1)
        tr = ScdaTrainer(mc.CFG, cuda, lr=1e-3, new_w=W, new_h=H, models=mc.seeded_models(build_product))
        src, tgt, gts, info = mc.seeded_inputs(H, W)
        np.random.seed(mc.SEEDS['numpy'])
        out = tr.step(src.to(cuda), gts, info, tgt.to(cuda), ignore_regions=regions)
        torch.cuda.synchronize()
        losses = {k: float(out[k]) for k in LOSSES}
        assert all(np.isfinite(v) for v in losses.values()), losses
        return losses, (_state_hash(tr) if want_hash else None), np.random.get_state()[1].copy()

    dev_losses, dev_hash, dev_rng = one_step(True, ign.to(cuda))
    np_losses, np_hash, np_rng = one_step(False, ign.to(cuda))
    assert dev_losses == np_losses
    assert dev_hash == np_hash
    np.testing.assert_array_equal(dev_rng, np_rng)
    plain_losses, _, _ = one_step(True, None, want_hash=False)
    assert any(plain_losses[k] != dev_losses[k] for k in ('rpn_cls', 'rpn_loc', 'rcnn_cls', 'rcnn_loc')), (plain_losses, dev_losses)
