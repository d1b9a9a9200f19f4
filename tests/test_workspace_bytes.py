"""The workspace sizes of the device evaluators and mask kernels, pinned on the CPU.  scda_*_workspace_bytes are host arithmetic over
the layouts of coco_eval.hip, map_eval.hip, mask_rle.hip and mask_poly.hip (the bump allocator of csrc/eval_prims.h), so the library
answers without a GPU.  tests/golden/workspace_bytes.json holds the answers of the build BEFORE the layouts moved onto the shared
allocator (tests/golden/make_golden_workspace_bytes.py writes it from `cases()`): a caller's buffer of yesterday's size must still fit."""
import json
import os

from conftest import ROOT
from scda_amd import native

GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
BIG = 0x7fffffff


def cases():
    """[(key, entry point, arguments)]"""
    out = []

    def add(fn, *sets):
        for args in sets:
            out.append(("%s(%s)" % (fn, ", ".join(str(a) for a in args)), "scda_%s_workspace_bytes" % fn, tuple(args)))

    # (n_images, D, K, A): the GPU tests' evaluators, scripts/time_coco_eval.py (5000 x 100, K = 80), n_images * D around one sort tile
    # (1024 rows), then the arguments that must give 0
    add("coco_accumulate", (6, 400, 3, 4), (1, 1024, 2, 4), (2, 1024, 2, 4), (3, 40, 255, 8), (3, 40, 4, 4), (4, 16, 4, 4), (3, 272, 3, 4),
        (2, 128, 4, 4), (3, 100, 80, 4), (5000, 100, 80, 4), (250, 100, 80, 4),
        (1, 1, 1, 4), (1, 1023, 1, 4), (1, 1024, 1, 4), (1, 1025, 1, 4), (1023, 1, 80, 4), (1025, 1, 80, 8), (41, 25, 255, 1),
        (0, 100, 80, 4), (1, 0, 80, 4), (1, 100, 0, 4), (1, 100, 80, 0), (1, 100, 80, 9), (-1, 100, 80, 4), (BIG, 1, 80, 4), (65536, 32768, 80, 4))
    # (n_images, D): tests/eval_edge_cases.py MAP_CAPS, scripts/time_map_eval.py (500 x 100)
    add("map_accumulate", (1, 1024), (2, 1024), (3, 320), (2, 4), (1, 4), (4, 100), (500, 100), (125, 100), (4, 300),
        (1, 1), (1, 1023), (1023, 1), (1024, 1), (1025, 1), (41, 25),
        (0, 100), (1, 0), (1, 1025), (-1, 100), (BIG, 1), (2097152, 1024))
    # (R, H, Wd, cap_runs): the 800 x 1344 planes of the RLE tests (Wd = 42) and small ones, cap_runs 0 and 1
    add("mask_rle", (1, 800, 42, 4096), (8, 800, 42, 1024), (100, 800, 42, 512), (400, 800, 42, 256), (3, 37, 3, 64), (1, 1, 1, 1),
        (1, 1, 1, 0), (5, 33, 2, 0), (5, 33, 2, 1), (65535, 1, 1, 1),
        (0, 800, 42, 16), (1, 0, 42, 16), (1, 800, 0, 16), (1, 800, 42, -1), (65536, 8, 1, 16), (1, 65536, 1, 16), (1, 8, 2048, 16),
        (1, 65535, 2047, 16))
    # (M, N, H, Wd)
    add("mask_iou", (100, 16, 800, 42), (128, 16, 64, 2), (1, 1, 1, 1), (100, 64, 512, 32), (3, 5, 37, 3), (65534, 1, 1, 1),
        (0, 1, 8, 1), (1, 0, 8, 1), (1, 1, 0, 1), (1, 1, 8, 0), (65535, 1, 8, 1), (1, 1, 65536, 1), (1, 1, 8, 2048))
    # (P, Q, H, Wd): no shape at all still gives a buffer that can be passed
    add("mask_frpoly", (0, 0, 5, 1), (1, 0, 800, 42), (0, 1, 800, 42), (40, 8, 800, 42), (7, 3, 37, 3), (1, 1, 1, 1), (300, 0, 512, 32),
        (-1, 0, 8, 1), (0, -1, 8, 1), (1, 1, 0, 1), (1, 1, 8, 0), (1, 1, 65536, 1), (1, 1, 65535, 2047))
    return out


def answers():
    return {key: int(getattr(native.lib(), fn)(*args)) for key, fn, args in cases()}


def test_workspace_bytes_match_the_recorded_ones():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = answers()
    assert sorted(got) == sorted(golden), "the case list and the golden file differ: rerun tests/golden/make_golden_workspace_bytes.py on the recorded build"
    moved = {k: (golden[k], v) for k, v in got.items() if golden[k] != v}
    assert not moved, "workspace sizes moved (recorded, now): %s" % moved


def test_the_recorded_cases_cover_both_answers():
    with open(GOLDEN) as f:
        golden = json.load(f)
    for fn in ("coco_accumulate", "map_accumulate", "mask_rle", "mask_iou", "mask_frpoly"):
        vals = [v for k, v in golden.items() if k.startswith(fn + "(")]
        assert 0 in vals and any(v > 0 for v in vals), fn
        assert all(v % 16 == 0 for v in vals), fn
