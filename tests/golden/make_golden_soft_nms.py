"""Generates tests/golden/soft_nms_ref.npz with the REFERENCE's own soft_nms: extensions/_cython_bbox/cython_nms.pyx:98-203 compiled
unmodified by oracle/build_ref.py into oracle/_ref/cython_nms.cpython-39-*.so.

Run with the interpreter that built it (the only one that can import it):
    python oracle/build_ref.py && /opt/conda/bin/python3.9 tests/golden/make_golden_soft_nms.py

The file holds reference OUTPUTS only, plus a sha256 of every seeded input (tests/soft_nms_cases.py regenerates the inputs
bit-identically under the system numpy and checks the digest): for every (method, parameter set) the cases of
soft_nms_cases.inputs_of back to back -- `counts` (rows returned per case), `inds` (the returned indices) and `scores` (the returned
score column).  The returned coordinates are asserted here to be the input's rows at `inds`, bit for bit, so the returned boxes are
input[inds] with that score column and storing them again would only store the inputs.

Nothing is compared under this interpreter: with numpy 1.26 the drop-in's host loop itself differs from the reference in the last
bit of the linear weight (`1 - np.float32` promotes to float64 there).  Every comparison runs under the system python."""
import glob
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import soft_nms_cases as sc  # noqa: E402


def load_ref():
    hits = glob.glob(os.path.join(ROOT, "oracle", "_ref", "cython_nms.cpython-39*.so"))
    assert hits, "run `python oracle/build_ref.py` first"
    if not hasattr(np, "int"):
        np.int = int
    spec = importlib.util.spec_from_file_location("cython_nms", hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    assert sys.version_info[:2] == (3, 9), "run with /opt/conda/bin/python3.9 (see the docstring)"
    ref = load_ref()
    made = {c: sc.make(*c) for c in sc.INPUTS}
    out = {"numpy_version": np.array(np.__version__), "input_sha256": np.array([sc.digest(made[c]) for c in sc.INPUTS])}
    for method in sc.METHODS:
        for pi, (sigma, Nt, threshold) in enumerate(sc.PARAMS):
            counts, inds, scores = [], [], []
            for c in sc.inputs_of(method, pi):
                a = made[c]
                before = a.copy()
                boxes, ii = ref.soft_nms(a, sigma, Nt, threshold, method)
                assert np.array_equal(a.view(np.uint32), before.view(np.uint32)), "the reference works on a copy"
                boxes, ii = np.asarray(boxes, dtype=np.float32), np.asarray(ii, dtype=np.int64)
                assert np.array_equal(boxes[:, :4].view(np.uint32), a[ii, :4].view(np.uint32)), "returned coordinates = input[inds]"
                assert len(set(ii.tolist())) == len(ii) and (len(ii) == 0 or (0 <= ii.min() and ii.max() < len(a)))
                counts.append(len(ii)); inds.append(ii.astype(np.uint16)); scores.append(boxes[:, 4].copy())
            key = "m%d_p%d_" % (method, pi)
            out[key + "counts"] = np.array(counts, dtype=np.int32)
            out[key + "inds"] = np.concatenate(inds)
            out[key + "scores"] = np.concatenate(scores)
            print("method %d (sigma %.1f, Nt %.1f, threshold %.3f): %3d cases, %6d of %6d rows returned"
                  % (method, sigma, Nt, threshold, len(counts), sum(counts), sum(c[0] for c in sc.inputs_of(method, pi))))
    path = os.path.join(HERE, "soft_nms_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
