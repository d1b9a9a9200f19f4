"""Ignore regions through the numpy paths of compute_anchor_targets / compute_proposal_targets (scda_amd/dropin/functions) against
tests/golden/ignore_regions_ref.npz, which the reference's own two functions produced on the cases of tests/ignore_region_cases.py
(tests/golden/make_golden_ignore_regions.py).  CPU only, the IoU hook pointed at the C oracle as in tests/test_host_functions.py;
bit-equal on every output, and the state of numpy's global generator afterwards too (the draws are part of the result).  The same
assertions run on the device paths in tests/test_ignore_regions_gpu.py."""
import os

import numpy as np
import pytest
import torch

import ignore_region_cases as IC
from oracle import native_ops as orc
from scda_amd.dropin import backend

CASES = IC.all_cases()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ignore_regions_ref.npz"))


@pytest.fixture()
def cpu_backend():
    backend.use(bbox_overlaps=lambda b, q: orc.bbox_overlaps(b[:, :4], q[:, :4]),
                nms=lambda d, t: torch.from_numpy(orc.nms(d.numpy(), t)))
    yield
    backend.reset()


def run_case(c, g, place=lambda a: torch.from_numpy(a)):
    """the case through the dropin function, inputs rebuilt from the golden file's own copies and put where `place` puts them;
    -> the outputs as host arrays, named as the golden names them"""
    from scda_amd.dropin.functions.anchor_target import compute_anchor_targets
    from scda_amd.dropin.functions.proposal_target import compute_proposal_targets
    n = c["name"]
    gts, ign, info = place(g[n + "/gts"]), place(g[n + "/ign"]), torch.from_numpy(g[n + "/info"])
    np.random.seed(c["seed"])
    if c["kind"] == "anchor":
        cls_t, loc_t, loc_m, norm = compute_anchor_targets(c["fs"], c["cfg"], gts, info, ign)
        assert cls_t.dtype == torch.int64 and loc_t.dtype == torch.float32 and loc_m.dtype == torch.float32
        assert cls_t.device == gts.device and loc_t.device == gts.device and loc_m.device == gts.device
        return {"cls_targets": cls_t.cpu().numpy(), "loc_targets": loc_t.cpu().numpy(), "loc_masks": loc_m.cpu().numpy(),
                "normalizer": np.int64(norm)}
    rois, labels, t, w = compute_proposal_targets(torch.from_numpy(g[n + "/props"]), c["cfg"], gts, info, ign)
    assert rois.dtype == torch.float32 and labels.dtype == torch.int64 and t.dtype == torch.float32 and w.dtype == torch.float32
    assert rois.device == gts.device and labels.device == gts.device and t.device == gts.device and w.device == gts.device
    return {"rois": rois.cpu().numpy(), "labels": labels.cpu().numpy(), "loc_targets": t.cpu().numpy(), "loc_weights": w.cpu().numpy()}


def assert_case_equals_golden(c, g, out):
    n = c["name"]
    for k, v in out.items():
        want = g[f"{n}/{k}"]
        assert v.shape == want.shape, (n, k, v.shape, want.shape)
        np.testing.assert_array_equal(v, want.astype(v.dtype), err_msg=f"{n}/{k}")
    IC.assert_rng_state(g, n)


def test_cases_file_matches_golden(golden):
    """the inputs the cases rebuild are the ones the reference was run on"""
    for c in CASES:
        for k in ("gts", "ign", "info", "props"):
            if k in c:
                np.testing.assert_array_equal(c[k], golden[f"{c['name']}/{k}"], err_msg=f"{c['name']}/{k}")
                assert c[k].dtype == np.float32


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_numpy_path_equals_reference(golden, cpu_backend, case):
    assert_case_equals_golden(case, golden, run_case(case, golden))
