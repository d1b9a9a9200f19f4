"""Soft-NMS on the MI355X at its structural edges (scda_amd/csrc/soft_nms.hip): the kernel against the reference's compiled soft_nms
on every hand-built case of tests/soft_nms_edge_cases.py (tests/golden/soft_nms_edges_ref.npz; tests/test_soft_nms_edges_rules.py
holds the host loop to the same cases) -- kept indices, their order and the final scores' bits, non-finite scores included -- and one
launch of five lists stored out of order over sentinel-filled outputs: what a list's sweep may write and what it must leave alone."""
import os

import numpy as np
import pytest
import torch

import soft_nms_edge_cases as ec
from gpu_arrays import bits

pytestmark = pytest.mark.gpu

SENTINEL = -7


@pytest.fixture(scope="module")
def edge_cases(golden_dir):
    return ec.load(os.path.join(golden_dir, "soft_nms_edges_ref.npz"))


def _launch(cuda, packed, seg, max_n, method, sigma, Nt, threshold):
    """the entry point itself over sentinel-filled keep / num -> (boxes after, keep, num) on the host"""
    from scda_amd import native as N
    b = torch.from_numpy(packed).to(cuda)
    s = torch.from_numpy(seg).to(cuda)
    keep = torch.full((max(len(packed), 1),), SENTINEL, dtype=torch.int64, device=cuda)
    num = torch.full((len(seg),), SENTINEL, dtype=torch.int64, device=cuda)
    st = N.lib().scda_soft_nms_segments_hip(N._p(b), N._p(s), len(seg), max_n, method, sigma, Nt, threshold, N._p(keep), N._p(num),
                                            N._stream())
    assert st == 0
    torch.cuda.synchronize()
    return b.cpu().numpy(), keep.cpu().numpy(), num.cpu().numpy()


@pytest.mark.parametrize("method,params", sorted({(m, c[2]) for c in ec.CASES for m in c[1]}))
def test_kernel_equals_reference_bit_for_bit(cuda, edge_cases, method, params):
    """all cases of one (method, parameter set) as the segments of ONE launch: counts, kept indices in selection order and the kept
    rows' score bits are the reference's; coordinates are never written and keep is written up to each list's count only"""
    cases = [c for c in edge_cases if c[1] == method and c[2] == params]
    assert cases
    lens = [len(c[3]) for c in cases]
    seg = np.zeros((len(cases), 3), dtype=np.int64)
    seg[:, 1] = lens
    seg[1:, 0] = np.cumsum(lens)[:-1]
    packed = np.concatenate([c[3] for c in cases], 0)
    boxes, keep, num = _launch(cuda, packed, seg, max(lens), method, *params)
    assert np.array_equal(bits(boxes[:, :4]), bits(packed[:, :4]))
    for (name, _, _, dets, want_boxes, want_inds), (first, n, _), k in zip(cases, seg, num):
        assert k == len(want_inds), (name, k, len(want_inds))
        got = keep[first:first + k]
        np.testing.assert_array_equal(got, want_inds, err_msg=name)
        assert np.array_equal(bits(boxes[first + got]), bits(want_boxes)), (name, boxes[first + got, 4], want_boxes[:, 4])
        assert (keep[first + k:first + n] == SENTINEL).all(), name


def _host(dets, method, params):
    from scda_amd.dropin.extensions._cython_bbox import cython_nms
    return cython_nms.soft_nms(dets, params[0], params[1], params[2], method)


@pytest.mark.parametrize("method", ec.ALL)
def test_five_lists_out_of_order_write_only_what_is_theirs(cuda, method):
    """S = 5 lists of lengths (0, 1, 64, 65, 3) whose rows lie in another order than their segments, gaps of foreign rows between
    them: each list is the host loop's result for it alone (the loop is held to the reference in test_soft_nms_edges_rules.py), keep
    beyond a list's count and everywhere outside the lists is untouched, as are all coordinates and every score of a row that was
    not kept; then max_n = 64, which cuts the 65-row list to its first 64 rows (include/scda_ops.h)"""
    params = ec.DEFAULT
    lists = [np.zeros((0, 5), np.float32), ec.cluster(1), ec.with_scores(64, {63: ec.NAN}), ec.cluster(65), ec.three_rows()]
    gap = np.array([[0, 0, 9, 9, 0.5]] * 2, dtype=np.float32)
    order = (3, 4, 0, 2, 1)                                             # where the lists lie, first to last
    seg = np.zeros((5, 3), dtype=np.int64)
    pieces, at = [gap], len(gap)
    for s in order:
        seg[s, :2] = (at, len(lists[s]))
        pieces += [lists[s], gap]
        at += len(lists[s]) + len(gap)
    packed = np.concatenate(pieces, 0)
    assert len(packed) == at and [int(n) for n in seg[:, 1]] == [0, 1, 64, 65, 3] and (np.diff(seg[:, 0]) < 0).any()
    for max_n in (65, 64):
        boxes, keep, num = _launch(cuda, packed, seg, max_n, method, *params)
        assert np.array_equal(bits(boxes[:, :4]), bits(packed[:, :4]))
        written = np.zeros(len(packed), bool)                           # keep entries and score rows a list's sweep may write
        kept_rows = np.zeros(len(packed), bool)
        for s in range(5):
            first, n = int(seg[s, 0]), min(int(seg[s, 1]), max_n)
            want_boxes, want_inds = _host(lists[s][:n], method, params)
            assert num[s] == len(want_inds), (s, max_n)
            got = keep[first:first + num[s]]
            np.testing.assert_array_equal(got, want_inds, err_msg="list %d, max_n %d" % (s, max_n))
            assert np.array_equal(bits(boxes[first + got]), bits(want_boxes)), (s, max_n)
            written[first:first + num[s]] = True
            kept_rows[first + got] = True
        assert (keep[~written] == SENTINEL).all()
        assert np.array_equal(bits(boxes[~kept_rows, 4]), bits(packed[~kept_rows, 4]))
        if max_n == 64:
            assert num[3] > 0 and not kept_rows[int(seg[3, 0]) + 64]       # the 65th row took no part
