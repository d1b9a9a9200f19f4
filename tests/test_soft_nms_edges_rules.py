"""Soft-NMS at its structural edges, the part that needs no GPU: the host loop of cython_nms.soft_nms against the reference's
compiled soft_nms on every hand-built case of tests/soft_nms_edge_cases.py (tests/golden/soft_nms_edges_ref.npz) -- disjoint lists,
all rows dead at once, deaths only in the head or only in the tail of a list, comparisons at equality, touching and inverted boxes,
non-finite scores and coordinates -- the rule set the HIP kernel is judged by in tests/test_soft_nms_edges_gpu.py."""
import os

import numpy as np
import pytest

import soft_nms_edge_cases as ec
from gpu_arrays import bits


@pytest.fixture(scope="module")
def edge_cases(golden_dir):
    return ec.load(os.path.join(golden_dir, "soft_nms_edges_ref.npz"))


def test_fixture_covers_the_case_list(edge_cases):
    assert [(c[0], c[1]) for c in edge_cases] == ec.KEYS
    names = {c[0] for c in edge_cases}
    for n in (64, 65, 129):
        assert "disjoint_n%d" % n in names
    for k in (1, 63, 64, 65):
        assert "head_k%d" % k in names and "tail_k%d" % k in names
    assert {"all_dead_n65", "all_dead_n129", "ov_eq_nt", "score_eq_thr", "score_eq_thr_next", "touching", "inverted", "nan_first",
            "nan_middle", "nan_last", "nan_three", "nan_beyond_64", "infinities", "nan_coord_in_t", "three_rows"} <= names


def test_the_cases_are_what_their_names_say(edge_cases):
    """the structure each case is built for, read off the reference's results"""
    got = {(name, m): (a, boxes, ii) for name, m, _, a, boxes, ii in edge_cases}
    for n in (64, 65, 129):                                             # nothing dies, nothing is rescored, ties by position
        for m in ec.ALL:
            a, boxes, ii = got[("disjoint_n%d" % n, m)]
            assert sorted(ii.tolist()) == list(range(n)) and np.array_equal(bits(boxes), bits(a[ii])) and (np.diff(boxes[:, 4]) <= 0).all()
            assert not np.array_equal(ii, np.argsort(-a[:, 4], kind="stable"))      # the swaps reorder equal scores: not a stable sort
    for n in (65, 129):
        a, boxes, ii = got[("all_dead_n%d" % n, 0)]
        assert ii.tolist() == [int(np.argmax(a[:, 4]))]
    for k in (1, 63, 64, 65):
        for m in ec.ALL:
            for head in (False, True):
                a, boxes, ii = got[("%s_k%d" % ("head" if head else "tail", k), m)]
                dying = set(range(1, 1 + k)) if head else set(range(1 + ec.SURVIVORS, 1 + ec.SURVIVORS + k))
                assert ii[0] == 0 and len(ii) == 1 + ec.SURVIVORS and not dying & set(ii.tolist())
    a, boxes, ii = got[("ov_eq_nt", 1)]                                  # ov == Nt: the score as it was; ov = 0.6: rescored
    assert boxes[ii.tolist().index(1), 4] == a[1, 4] and boxes[ii.tolist().index(2), 4] < a[2, 4]
    assert 1 in got[("ov_eq_nt", 0)][2] and 2 not in got[("ov_eq_nt", 0)][2]
    a, boxes, ii = got[("score_eq_thr", 1)]                              # a rescored score equal to the threshold stays ...
    assert boxes[ii.tolist().index(1), 4] == np.float32(0.125)
    assert 1 not in got[("score_eq_thr_next", 1)][2]                     # ... and dies under the next float32
    for m in ec.ALL:
        ii = got[("touching", m)][2]
        assert set(ii.tolist()) == {0, 1, 2, 3, 5}                       # row 4 (iw == 1) was examined and died
        assert got[("three_rows", m)][2].tolist()[:2] == [2, 1]
    assert got[("three_rows", 0)][2].tolist() == [2, 1]
    assert got[("nan_first", 0)][2][0] == 0 and np.isnan(got[("nan_first", 0)][1][0, 4])       # a NaN at i is selected ...
    for (name, m), (a, boxes, ii) in got.items():                        # the NaN-coordinate cases form no NaN score (see nan_coord)
        if name.startswith("nan_coord"):
            assert not np.isnan(boxes[:, 4]).any(), (name, m)
    a, boxes, ii = got[("nan_coord_in_other", 0)]                        # never touched: even the one below the threshold stays
    assert {2, 7} <= set(ii.tolist()) and boxes[ii.tolist().index(2), 4] == a[2, 4] < 0.001
    ii = got[("nan_middle", 0)][2]                                       # ... and anywhere else only when it is all that is left
    assert 5 in ii and ii[0] != 5


def test_host_loop_equals_reference_bit_for_bit(edge_cases):
    from scda_amd.dropin.extensions._cython_bbox import cython_nms
    for name, method, (sigma, Nt, threshold), dets, want_boxes, want_inds in edge_cases:
        before = dets.copy()
        boxes, inds = cython_nms.soft_nms(dets, sigma, Nt, threshold, method)
        where = "%s, method %d" % (name, method)
        assert before.tobytes() == dets.tobytes(), where
        np.testing.assert_array_equal(np.asarray(inds), want_inds, err_msg=where)
        assert boxes.dtype == np.float32
        np.testing.assert_array_equal(bits(boxes), bits(want_boxes), err_msg=where)
