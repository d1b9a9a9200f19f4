"""Generates tests/golden/bbox_overlaps_live.npz with the REFERENCE's own bbox_overlaps: extensions/_cython_bbox/cython_bbox.pyx
compiled unmodified by oracle/build_ref.py into oracle/_ref/:

    python oracle/build_ref.py && python tests/golden/make_golden_bbox_live.py

The inputs are the seeded random boxes of tests/test_oracle_golden.py::test_bbox_overlaps_matches_live_reference_build (regenerated
there, checked against the sha256 stored here); the file holds the reference's outputs and those digests."""
import glob
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    from test_oracle_golden import live_cases
    hits = glob.glob(os.path.join(ROOT, "oracle", "_ref", "cython_bbox*.so"))
    assert hits, "run `python oracle/build_ref.py` first"
    spec = importlib.util.spec_from_file_location("cython_bbox", hits[0])
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for i, (boxes, query) in enumerate(live_cases()):
        out["case%d_sha256" % i] = np.array(hashlib.sha256(boxes.tobytes() + query.tobytes()).hexdigest())
        out["case%d_out" % i] = ref.bbox_overlaps(boxes, query)
    np.savez_compressed(os.path.join(HERE, "bbox_overlaps_live.npz"), **out)
    print(sorted(out))


if __name__ == "__main__":
    main()
