"""Generates tests/golden/soft_nms_edges_ref.npz with the REFERENCE's own soft_nms (extensions/_cython_bbox/cython_nms.pyx:98-203
compiled unmodified by oracle/build_ref.py into oracle/_ref/cython_nms.cpython-39-*.so) on the hand-built edge lists of
tests/soft_nms_edge_cases.py.

Run with the interpreter that built it (the only one that can import it):
    python oracle/build_ref.py && /opt/conda/bin/python3.9 tests/golden/make_golden_soft_nms_edges.py

The file holds reference OUTPUTS only, plus a sha256 of every input: for every (case, method) of soft_nms_edge_cases.KEYS back to
back `counts` (rows returned), `inds` (the returned indices) and `score_bits` (the returned score column as uint32 words: some are
NaN).  The returned coordinates are asserted here to be the input's rows at `inds`, bit for bit.  Nothing is compared under this
interpreter (see make_golden_soft_nms.py); every comparison runs under the system python."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import soft_nms_edge_cases as ec  # noqa: E402
from make_golden_soft_nms import load_ref  # noqa: E402


def main():
    assert sys.version_info[:2] == (3, 9), "run with /opt/conda/bin/python3.9 (see the docstring)"
    ref = load_ref()
    counts, inds, scores = [], [], []
    for name, methods, (sigma, Nt, threshold), a in ec.CASES:
        for method in methods:
            before = a.copy()
            boxes, ii = ref.soft_nms(a, sigma, Nt, threshold, method)
            assert before.tobytes() == a.tobytes(), "the reference works on a copy"
            boxes, ii = np.asarray(boxes, dtype=np.float32), np.asarray(ii, dtype=np.int64)
            assert np.array_equal(boxes[:, :4].view(np.uint32), a[ii, :4].view(np.uint32)), "returned coordinates = input[inds]"
            assert len(set(ii.tolist())) == len(ii) and (len(ii) == 0 or (0 <= ii.min() and ii.max() < len(a)))
            counts.append(len(ii)); inds.append(ii.astype(np.uint16)); scores.append(boxes[:, 4].copy().view(np.uint32))
            print("%-24s method %d: %3d of %3d rows returned" % (name, method, len(ii), len(a)))
    out = {"numpy_version": np.array(np.__version__), "keys": np.array(["%s/m%d" % k for k in ec.KEYS]),
           "input_sha256": np.array([ec.digest(c[3]) for c in ec.CASES]), "counts": np.array(counts, dtype=np.int32),
           "inds": np.concatenate(inds), "score_bits": np.concatenate(scores)}
    path = os.path.join(HERE, "soft_nms_edges_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
