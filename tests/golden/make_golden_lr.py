"""Generates tests/golden/lr_warmup_ref.npz with the REFERENCE's own per-iteration warm-up scheduler (utils/lr_helper.py
IterExponentialLR, imported unmodified from the reference checkout) driving this repository's FlatAdam:

    SCDA_REFERENCE=<reference checkout> python tests/golden/make_golden_lr.py

The file holds what tests/test_lr_schedule.py::test_iter_exponential_warmup[reference] compares the product's scheduler with:
the learning rate and initial_lr after construction, the learning rate after each of 4 steps, and whether a non-Optimizer
argument is refused with TypeError."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF = os.environ.get("SCDA_REFERENCE", "/root/reference")


def main():
    from scda_amd.lr_schedule import warmup_gamma
    from test_lr_schedule import small_flat
    spec = importlib.util.spec_from_file_location("ref_lr_helper", os.path.join(REF, "utils", "lr_helper.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    net, flat, opt = small_flat()
    gamma = warmup_gamma(8, 1, 4)
    s = mod.IterExponentialLR(opt, gamma)
    out = {"gamma": np.float64(gamma), "lr0": np.float64(opt.param_groups[0]['lr']),
           "initial_lr": np.float64(opt.param_groups[0]['initial_lr'])}
    seen = []
    for _ in range(4):
        s.step()
        seen.append(opt.param_groups[0]['lr'])
    out["seen"] = np.array(seen, np.float64)
    try:
        mod.IterExponentialLR(object(), gamma)
        out["type_error"] = np.bool_(False)
    except TypeError:
        out["type_error"] = np.bool_(True)
    np.savez(os.path.join(HERE, "lr_warmup_ref.npz"), **out)
    print({k: v.tolist() for k, v in out.items()})


if __name__ == "__main__":
    main()
