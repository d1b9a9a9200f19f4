"""tests/roi_refs.py (the plain references the GPU edge suite compares the HIP kernels with) pinned against the C oracle
(oracle/scda_oracle.c), on seeded random cases and on the edge cases of tests/roi_edge_cases.py.  CPU only."""
import numpy as np
import pytest

import np_restate as npr
import roi_edge_cases as K
import roi_refs as R
from oracle import native_ops as orc

f32 = np.float32
SCALE = K.SCALE


def assert_same(a, b, msg=""):
    """bit for bit (NaN only where the other side has one; inf and signed values compare as values)"""
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=msg)


# ---------------------------------------------------------------- RoI max pooling
def pool_cases():
    rs = np.random.RandomState(31)
    shape = (2, 3, 20, 27)
    yield "random", K.tied_features(rs, shape), K.rand_rois(rs, 40, 2, 20, 27)
    for axis in "wh":
        for clip in (False, True):
            feat, rois = K.sweep_case(axis, clip)
            yield "sweep_%s%s" % (axis, "_clip" if clip else ""), feat, rois
    feat, rois = K.sweep_case_large()
    yield "sweep_large", feat, rois
    for name, feat, rois in K.special_pool_cases():
        yield "special_" + name, feat, rois


@pytest.mark.parametrize("pooled", [(1, 1), (2, 3), (3, 2), (7, 7), (8, 8), (9, 8), (14, 14)])
def test_roi_pool_restatements_equal_the_oracle(pooled):
    PH, PW = pooled
    for name, feat, rois in pool_cases():
        if name.startswith("sweep") and pooled not in ((7, 7), (14, 14)):
            continue
        eo, ea = orc.roi_pool_fwd(feat, rois, PH, PW, SCALE)
        out, arg = R.roi_pool_fwd(feat, rois, PH, PW, SCALE)
        assert_same(out, eo, name); assert_same(arg, ea, name)
        top = np.random.RandomState(7).randn(*eo.shape).astype(f32)
        want = orc.roi_pool_bwd(top, ea, rois, feat.shape, PH, PW, SCALE)            # the C gather, roi_pooling_kernel.cu:128-203
        assert_same(R.roi_pool_bwd_reference_rule(top, ea, rois, feat.shape, PH, PW, SCALE), want, name)
        assert_same(orc.roi_pool_bwd_scatter(top, ea, feat.shape, PH, PW, rois, SCALE), want, name)
        assert_same(orc.roi_pool_bwd_scatter(top, ea, feat.shape, PH, PW), R.roi_pool_bwd_pure_scatter(top, ea, feat.shape), name)   # without RoIs: ungated
        if ea.size <= 20000:
            assert_same(npr.roi_pool_bwd_scatter(top, ea, feat.shape, rois, SCALE), want, name)    # the explicit fp32 loop


def test_ordered_scatter_adds_in_index_order():
    """np.add.at on float32 adds one contributor at a time, front to back: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 does not"""
    arg = np.zeros((1, 1, 1, 3), np.int32)
    for top, want in (([2.0 ** 24, 1, 1], 2.0 ** 24), ([1, 1, 2.0 ** 24], 2.0 ** 24 + 2)):
        assert R.roi_pool_bwd_pure_scatter(np.array(top, f32).reshape(1, 1, 1, 3), arg, (1, 1, 1, 1))[0, 0, 0, 0] == f32(want)


@pytest.mark.parametrize("axis", ["w", "h"])
def test_last_bin_reaches_one_pixel_past_the_roi_and_the_reference_drops_its_gradient(axis):
    """fl(57 / 7) * 7 > 57 in fp32 (likewise 114, 121): the forward's last window ends at ew + 1 (roi_pooling_kernel.cu:54-61).  On
    features that increase along that axis the argmax of the last bin IS pixel ew + 1; the reference's backward only visits RoIs whose
    rectangle [sw..ew] holds the pixel (:161-166), so that pixel gets nothing; a scatter driven by argmax alone would add it.
    (roi_pool_py.py computes the bin size in Python doubles, where the last window ends at ew: tests/roipool_cases.py keeps these
    extents out of the vectors recorded from it, so no golden file can show this; the C oracle follows the kernel text.)"""
    feat, rois = K.sweep_case(axis, clip=False)
    B, C, H, W = feat.shape
    out, arg = R.roi_pool_fwd(feat, rois, 7, 7, SCALE)
    top = np.ones_like(out)
    rule = R.roi_pool_bwd_reference_rule(top, arg, rois, feat.shape, 7, 7, SCALE)
    pure = R.roi_pool_bwd_pure_scatter(top, arg, feat.shape)
    seen = set()
    for n, roi in enumerate(rois):
        s, e_end = (int(roi[1] / 16), int(roi[3] / 16)) if axis == "w" else (int(roi[2] / 16), int(roi[4] / 16))
        extent = e_end - s + 1
        a = arg[n, 0, 6, 6] if axis == "w" else arg[n, 0, 6, 6]
        pos = (a % W) if axis == "w" else (a // W) % H
        if extent in (57, 114, 121):
            assert pos == e_end + 1, (extent, pos, e_end)
            seen.add(extent)
        else:
            assert pos == e_end, (extent, pos, e_end)
    assert seen == {57, 114, 121}
    differs = np.argwhere(rule != pure)
    assert len(differs) > 0
    for b, c, h, w in differs:
        assert rule[b, c, h, w] == 0 or rule[b, c, h, w] < pure[b, c, h, w]
    # the pixel past the 57-extent RoI that starts at 5 (pixel 62) lies inside no other RoI's last bin... but inside wider RoIs'
    # rectangles; what is asserted is the rule itself: a dropped argmax contributes to `pure` only
    n57 = [n for n, roi in enumerate(rois) if (roi[3] - roi[1] if axis == "w" else roi[4] - roi[2]) == 56 * 16]
    only = np.zeros_like(top); only[n57] = 1.0
    rule57 = R.roi_pool_bwd_reference_rule(only, arg, rois, feat.shape, 7, 7, SCALE)
    pure57 = R.roi_pool_bwd_pure_scatter(only, arg, feat.shape)
    for n in n57:
        a = arg[n, 0, 6, 6]
        assert rule57.reshape(-1)[a] == 0 and pure57.reshape(-1)[a] > 0
    # with the pixel past the RoI clipped away by the map's edge the two agree
    feat, rois = K.sweep_case(axis, clip=True)
    out, arg = R.roi_pool_fwd(feat, rois, 7, 7, SCALE)
    top = np.ones_like(out)
    assert_same(R.roi_pool_bwd_reference_rule(top, arg, rois, feat.shape, 7, 7, SCALE), R.roi_pool_bwd_pure_scatter(top, arg, feat.shape))


def test_gather_bin_range_never_misses_a_pixel_inside_the_roi():
    """the scatter form applies the `in_roi` gate but not the gather's phstart .. phend range (:182-190); that is the same thing only
    if the range of an in-RoI pixel always holds every bin whose forward window holds the pixel.  One axis, extents 1 .. 336, every
    pooled size the scatter form takes in the tests: no miss.  (The pixel PAST the RoI is the one the gate is for.)"""
    for P in (1, 2, 3, 6, 7, 8, 14):
        p = np.arange(P, dtype=f32)
        for e in range(1, 337):
            b = f32(e) / f32(P)
            start = np.floor(p * b).astype(np.int64); end = np.ceil((p + f32(1)) * b).astype(np.int64)     # forward windows
            x = np.arange(e, dtype=f32)
            lo = np.clip(np.floor(x / b), 0, P).astype(np.int64); hi = np.clip(np.ceil((x + f32(1)) / b), 0, P).astype(np.int64)
            xi = np.arange(e)[:, None]
            in_window = (xi >= start[None, :]) & (xi < end[None, :])
            in_range = (np.arange(P)[None, :] >= lo[:, None]) & (np.arange(P)[None, :] < hi[:, None])
            assert not (in_window & ~in_range).any(), (P, e)
            assert end[-1] in (e, e + 1) and (end[-1] == e or P in (7, 14))


# ---------------------------------------------------------------- RoIAlign
def align_cases():
    rs = np.random.RandomState(32)
    yield "random_8x8", rs.randn(2, 3, 13, 9).astype(f32), K.align_inexact_rois(rs, 33, 2, 13, 9), 8, 8, SCALE
    yield "random_2x9", rs.randn(2, 3, 13, 9).astype(f32), K.align_inexact_rois(rs, 20, 2, 13, 9), 2, 9, SCALE
    yield "pile", rs.randn(1, 2, 6, 7).astype(f32), K.align_inexact_rois(rs, 310, 1, 6, 7, pile=300), 7, 7, SCALE
    yield "geometry_2x2", rs.randn(1, 2, 6, 7).astype(f32), K.align_geometry_rois(6, 7), 2, 2, 1.0
    yield "geometry_3x3", rs.randn(1, 2, 6, 7).astype(f32), K.align_geometry_rois(6, 7), 3, 3, 1.0
    yield "map_2x2", rs.randn(1, 2, 2, 2).astype(f32), K.align_inexact_rois(rs, 12, 1, 2, 2), 7, 7, SCALE


def test_roi_align_statement_equals_the_oracle_to_fp32_rounding():
    for name, feat, rois, AH, AW, scale in align_cases():
        want = orc.roi_align_fwd(feat, rois, AH, AW, scale)
        ref = R.roi_align(feat, rois, AH, AW, scale)
        # the oracle evaluates the same double expression (products left to right) and rounds once: at most one fp32 rounding of the
        # result plus double-rounding noise
        assert np.abs(want - ref).max() <= 2.0 ** -24 * np.abs(ref).max() * (1 + 1e-6), name
        assert_same(ref == 0, want == 0, name)              # the same samples are outside
        top = K.signed_unit_tops(np.random.RandomState(3), want.shape)
        _, g, k, S, wts = R.roi_align(feat, rois, AH, AW, scale, top, stats=True)
        og = orc.roi_align_bwd(top, rois, feat.shape, AH, AW, scale)
        assert (np.abs(og - g) <= (k + 2) * 2.0 ** -24 * S).all(), name
        assert ((k == 0) == (S == 0)).all() and (g[k == 0] == 0).all()
    _, _, k, S, wts = R.roi_align(np.zeros((1, 1, 6, 7), f32), np.array([[0, 16, 16, 48, 48]], f32), 2, 2, SCALE, np.ones((1, 1, 2, 2), f32), stats=True)
    assert k.sum() == 4 and S.sum() == 4.0 and sorted(wts) == [0.0] * 12 + [1.0] * 4     # samples on pixel centres: one corner each


def test_roi_align_nan_coordinate_statement():
    feat = np.random.RandomState(4).randn(1, 1, 6, 7).astype(f32)
    rois = np.array([[0, np.nan, 16, 48, 48], [0, 16, 16, 48, np.nan], [0, 16, 16, 48, 48]], f32)
    want = orc.roi_align_fwd(feat, rois, 3, 3, SCALE)
    ref = R.roi_align(feat, rois, 3, 3, SCALE)
    assert_same(np.isnan(ref), np.isnan(want))
    assert np.isnan(want[0]).all() and not np.isnan(want[2]).any()


@pytest.mark.parametrize("grid", [(2, 2), (7, 7), (8, 8), (15, 15), (16, 17)])
def test_roi_align_exact_backward_is_exact(grid):
    """the construction of the exact backward cases: every contribution a multiple of 1/64, every sum below 2^24 / 64 -- so the
    oracle's fp32 sums (one order) equal the fp64 statement bit for bit, and so must any other order"""
    AH, AW = grid
    rs = np.random.RandomState(AH * 17 + AW)
    shape = (2, 3, 13, 9)
    rois = K.align_exact_rois(rs, 33, 2, 13, 9, AH, AW)
    top = rs.randint(-64, 65, (33, 3, AH, AW)).astype(f32)
    _, g, k, S, wts = R.roi_align(np.zeros(shape, f32), rois, AH, AW, SCALE, top, stats=True)
    assert (wts * 64 == np.round(wts * 64)).all() and S.max() < 2.0 ** 24 / 64 and k.max() > 4
    assert (wts > 0).sum() > 0.2 * wts.size                      # not all samples outside / on pixel centres
    assert_same(orc.roi_align_bwd(top, rois, shape, AH, AW, SCALE), g.astype(f32))


def test_roi_align_refuses_features_past_int32():
    """B*C*H*W > 2^31 - 1 overflows the int corner index: refused on the shape alone, before any pointer is looked at"""
    from scda_amd import native
    lib = native.lib()
    for fn in (lib.scda_roi_align_fwd_hip, lib.scda_roi_align_cmajor_fwd_hip, lib.scda_roi_align_bwd_hip, lib.scda_roi_align_cmajor_bwd_hip):
        assert fn(None, None, 4, 2, 1024, 1024, 1024, 7, 7, 0.0625, None, None) != 0
        assert b"int32" in lib.scda_last_error()
        assert fn(None, None, 0, 1, 2047, 1024, 1024, 7, 7, 0.0625, None, None) == 0      # below the limit, no RoI: nothing to do


# ---------------------------------------------------------------- focal losses
@pytest.mark.parametrize("rows,C", [(1, 8), (257, 8), (257, 1), (257, 2), (257, 81)])
@pytest.mark.parametrize("gamma,alpha,wp", [(2.0, 0.25, 97.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.5), (2.0, 1.0, 0.0), (0.5, 0.25, 0.5)])
def test_focal_formulas_equal_the_oracle(rows, C, gamma, alpha, wp):
    x, t = K.focal_case(rows, C, softmax=False)
    for fn in ("focal_sigmoid_fwd", "focal_sigmoid_bwd"):
        ref = getattr(R, fn)(x, t, wp, gamma, alpha, C)
        got = getattr(orc, fn)(x, t, wp, gamma, alpha, C)
        assert np.isfinite(ref).all() and np.isfinite(got).all(), fn
        np.testing.assert_allclose(got, ref, atol=1e-6, rtol=1e-5, err_msg=fn)
    x, t = K.focal_case(rows, C, softmax=True)
    rl, rp = R.focal_softmax_fwd(x, t, wp, gamma, alpha, C)
    ol, op = orc.focal_softmax_fwd(x, t, wp, gamma, alpha, C)
    np.testing.assert_allclose(op, rp, atol=1e-6)
    np.testing.assert_allclose(ol, rl, atol=1e-6, rtol=1e-5)
    rg = R.focal_softmax_bwd(op, t, wp, gamma, alpha, C)
    og = orc.focal_softmax_bwd(x, t, op, wp, gamma, alpha, C)
    assert not np.isnan(og).any() and not np.isnan(ol).any()
    ok = np.isfinite(rg)
    assert ok.all() or gamma < 1          # gamma < 1: (1 - p)^(gamma - 1) overflows where 0 < 1 - p is tiny
    np.testing.assert_allclose(og[ok], rg[ok], atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------- overlaps
@pytest.mark.parametrize("n1,n2,sz", [(1, 1, 4), (37, 23, 4), (37, 23, 5), (300, 1, 4), (1, 300, 5)])
def test_overlap_restatements_equal_the_oracle(n1, n2, sz):
    a, b = K.overlap_case(n1, n2, sz)
    assert_same(R.iou_overlaps(a, b), orc.iou_overlaps(a, b))
    assert_same(R.bbox_overlaps(a[:, :4], b[:, :4]), orc.bbox_overlaps(np.ascontiguousarray(a[:, :4]), np.ascontiguousarray(b[:, :4])))
    if n1 > 20:
        o = orc.iou_overlaps(a, b)
        assert (o == 0).any() and (o > 0).any()
