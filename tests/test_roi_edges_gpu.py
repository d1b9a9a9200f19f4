"""The RoI pooling, RoIAlign, focal-loss and overlap kernels of scda_amd/csrc/detection_ops.hip at their edges: every launch path of the C
ABI (per-RoI / per-element forward, scatter / gather backward, plane / atomic RoIAlign backward, both RoIAlign layouts, grid-stride
second sweeps), the shapes on either side of each switch, and the values and RoIs where the operators' definitions have corners.

Expected values are the plain references of tests/roi_refs.py (pinned against the C oracle by tests/test_roi_refs.py) and the C oracle
itself.  RoI pooling, the overlaps and the exact RoIAlign backward compare bit for bit.  Tolerance rule elsewhere, as in
tests/test_nn_ops_edges_gpu.py: with ref64 the fp64 statement on the fp32 inputs and o32 the C oracle's fp32 result,
    E32 = max|o32 - ref64| / max|ref64|,     max|kernel - ref64| / max|ref64| <= max(4 E32, 4 * 2^-23);
the inexact RoIAlign backward has a per-pixel bound of its own (see there).  Each tolerance case prints an `EDGE ...` line (pytest -s)."""
import numpy as np
import pytest
import torch

import roi_edge_cases as K
import roi_refs as R
from oracle import native_ops as orc

pytestmark = pytest.mark.gpu

f32 = np.float32
ULP4 = 4.0 * 2.0 ** -23
SCALE = K.SCALE


def dev(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(cuda).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, msg=""):
    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg=msg)


def check(case, got, ref64, o32, ok=None):
    """the tolerance rule; `ok` restricts it to the elements where the fp64 statement is finite"""
    got, ref, o32 = np.asarray(got, np.float64), np.asarray(ref64, np.float64), np.asarray(o32, np.float64)
    assert got.shape == ref.shape == o32.shape, (case, got.shape, ref.shape)
    if ok is not None:
        got, ref, o32 = got[ok], ref[ok], o32[ok]
    assert np.isfinite(ref).all(), case
    scale = float(np.abs(ref).max()) if ref.size else 1.0
    scale = scale or 1.0
    e32 = float(np.abs(o32 - ref).max()) / scale if ref.size else 0.0
    err = float(np.abs(got - ref).max()) / scale if ref.size else 0.0
    bound = max(4.0 * e32, ULP4)
    print(f"\nEDGE {case} E32={e32:.3e} kernel={err:.3e} bound={bound:.3e}")
    assert err <= bound, f"{case}: kernel error {err:.3e} over {bound:.3e} (E32 {e32:.3e})"


# ================================================================ RoI max pooling
def pool_fwd_bwd(cuda, feat, rois, PH, PW, name, scale=SCALE, seed=7):
    """forward values and argmax, and the backward on that argmax, bit for bit against roi_refs"""
    from scda_amd import native
    want, warg = R.roi_pool_fwd(feat, rois, PH, PW, scale)
    out, arg = native.roi_pool_fwd(dev(feat, cuda), dev(rois, cuda), PH, PW, scale)
    same(host(out), want, name + " values"); same(host(arg), warg, name + " argmax")
    top = np.random.RandomState(seed).randn(*want.shape).astype(f32)
    g = host(native.roi_pool_bwd(dev(top, cuda), arg, dev(rois, cuda), feat.shape, PH, PW, scale))
    same(g, R.roi_pool_bwd_reference_rule(top, warg, rois, feat.shape, PH, PW, scale), name + " backward")
    return want, warg, g


@pytest.mark.parametrize("axis", ["w", "h"])
@pytest.mark.parametrize("clip", [False, True], ids=["inside", "clipped"])
def test_roi_pool_extent_sweep_scatter_form(cuda, axis, clip):
    """RoI extents 1 .. 122 on planes of 1040 pixels (the ordered-scatter backward).  For extents 57, 114 and 121 the last 7-bin window
    ends one pixel past the RoI (fp32 bin size); on these increasing features that pixel is the argmax, and the reference's backward
    gives it nothing (tests/test_roi_refs.py states this on the CPU).  `clipped`: the RoIs end on the map's last pixel."""
    feat, rois = K.sweep_case(axis, clip)
    want, warg, g = pool_fwd_bwd(cuda, feat, rois, 7, 7, f"sweep {axis}")
    top = np.random.RandomState(7).randn(*want.shape).astype(f32)
    differs = (g != R.roi_pool_bwd_pure_scatter(top, warg, feat.shape)).any()
    assert differs == (not clip)          # the case under test occurs exactly where the pixel past the RoI exists


def test_roi_pool_extent_sweep_gather_form(cuda):
    """the same extents, along both axes, on a plane of 64 x 130 = 8320 pixels: too large for the scatter form's LDS (8192)"""
    feat, rois = K.sweep_case_large()
    want, warg, g = pool_fwd_bwd(cuda, feat, rois, 7, 7, "sweep 64x130")
    top = np.random.RandomState(7).randn(*want.shape).astype(f32)
    assert (g != R.roi_pool_bwd_pure_scatter(top, warg, feat.shape)).any()


@pytest.mark.parametrize("pooled", [(1, 1), (2, 3), (3, 2), (7, 7), (8, 8), (9, 8), (14, 14)], ids=lambda p: "%dx%d" % p)
def test_roi_pool_pooled_sizes(cuda, pooled):
    """8 x 8 = 64 bins is the scatter backward's limit (lane = bin), 9 x 8 and 14 x 14 take the gather form; 7 x 7 is the templated forward"""
    rs = np.random.RandomState(31)
    feat, rois = K.tied_features(rs, (2, 3, 20, 27)), K.rand_rois(rs, 40, 2, 20, 27)
    pool_fwd_bwd(cuda, feat, rois, pooled[0], pooled[1], "pooled %dx%d" % pooled)


def test_roi_pool_per_element_kernel_equals_per_roi_kernel(cuda):
    """R = 65536 is past the grid's y limit and takes roi_pool_fwd_kernel (one thread per output); R = 65535 takes the per-RoI kernel:
    identical rows for identical RoIs, and both equal the restatement"""
    from scda_amd import native
    rs = np.random.RandomState(33)
    feat = K.tied_features(rs, (1, 1, 4, 4))
    base = np.concatenate([K.rand_rois(rs, 60, 1, 4, 4), [[0, -64, 0, -32, 16], [0, 16, 16, 0, 0], [0, 0, 0, 63, 63], [0, 8, 8, 24, 24]]]).astype(f32)
    want, warg = R.roi_pool_fwd(feat, base, 2, 2, SCALE)
    pick = np.arange(65536) % len(base)
    pick[65535] = 0
    rois = np.ascontiguousarray(base[pick])
    d_feat, d_rois = dev(feat, cuda), dev(rois, cuda)
    out_e, arg_e = native.roi_pool_fwd(d_feat, d_rois, 2, 2, SCALE)
    out_r, arg_r = native.roi_pool_fwd(d_feat, d_rois[:65535].contiguous(), 2, 2, SCALE)
    same(host(out_e), want[pick]); same(host(arg_e), warg[pick])
    same(host(out_r), want[pick[:65535]]); same(host(arg_r), warg[pick[:65535]])
    assert torch.equal(out_e[:65535], out_r) and torch.equal(arg_e[:65535], arg_r) and torch.equal(out_e[65535], out_e[0])


def test_roi_pool_per_roi_kernel_past_its_workgroup_cap(cuda):
    """C = 340 at 7 x 7: 16660 outputs per RoI = 65.08 workgroups of 256, capped at 64: a second sweep with a tail of 276"""
    rs = np.random.RandomState(34)
    feat = K.tied_features(rs, (1, 340, 6, 9))
    rois = np.array([[0, 3, 5, 130, 90], [0, 40, 20, 60, 30]], f32)
    pool_fwd_bwd(cuda, feat, rois, 7, 7, "C=340")


@pytest.mark.parametrize("hw", [(2, 3), (13, 9), (64, 128), (3, 2731)], ids=lambda s: "%dx%d" % s)
def test_roi_pool_bwd_plane_sizes(cuda, hw):
    """planes of 6 pixels (the last of the eight slices is empty: span -1), 117 (no multiple of 8), 8192 (exactly 96 KB of LDS: the
    last the scatter form takes) and 8193 (gather form); R on either side of the 32-RoI staging chunk; image 1 of 3 has no RoI"""
    from scda_amd import native
    H, W = hw
    shape = (3, 2, H, W)
    rs = np.random.RandomState(H * W)
    feat = K.tied_features(rs, shape)
    for Rn in (0, 1, 31, 32, 33, 65):
        rois = K.rand_rois(rs, Rn, 2, H, W) if Rn else np.zeros((0, 5), f32)
        rois[:, 0] *= 2                                                     # images 0 and 2
        if Rn == 0:
            g = native.roi_pool_bwd(torch.zeros(0, 2, 7, 7, device=cuda), torch.zeros(0, 2, 7, 7, dtype=torch.int32, device=cuda),
                                    torch.zeros(0, 5, device=cuda), shape, 7, 7, SCALE)
        else:
            g = torch.from_numpy(pool_fwd_bwd(cuda, feat, rois, 7, 7, f"{H}x{W} R={Rn}", seed=Rn)[2])
            assert Rn < 31 or (float(g[0].abs().sum()) > 0 and float(g[2].abs().sum()) > 0)
        assert g.shape == shape and float(g[1].abs().max()) == 0.0 and not torch.signbit(g[1]).any()


def test_roi_pool_bwd_refuses_what_the_gather_form_cannot_stage(cuda):
    """72 bins take the gather form, whose RoI list lives in 64 KB of LDS: 3277 RoIs x 20 bytes do not fit -- refused before any launch"""
    from scda_amd import native
    Rn = 3277
    top = torch.zeros(Rn, 1, 9, 8, device=cuda)
    arg = torch.full((Rn, 1, 9, 8), -1, dtype=torch.int32, device=cuda)
    with pytest.raises(native.ScdaNativeError, match="too large"):
        native.roi_pool_bwd(top, arg, torch.zeros(Rn, 5, device=cuda), (1, 1, 4, 4), 9, 8, SCALE)


@pytest.mark.parametrize("pooled", [(2, 2), (7, 7)], ids=lambda p: "%dx%d" % p)
def test_roi_pool_special_values_and_rois(cuda, pooled):
    """a constant window (the first pixel in scan order wins); windows of -inf / -FLT_MAX / NaN only (nothing is > -FLT_MAX: value
    -FLT_MAX, argmax -1, no gradient); NaN and +inf among numbers (NaN never wins, +inf does); RoIs wholly outside on each side
    (0, -1), half outside, inverted (width 1), and corners on .5 (half away from zero)"""
    for name, feat, rois in K.special_pool_cases():
        want, warg, g = pool_fwd_bwd(cuda, feat, rois, pooled[0], pooled[1], name)
        assert not np.isnan(want).any() and not np.isnan(g).any()
        for n in (2, 3, 4, 5):
            assert (want[n] == 0).all() and (warg[n] == -1).all(), (name, n)
        if name == "constant":
            assert warg[0, 0, 0, 0] == 0 and (want[[0, 1, 10, 11]] == 2.0).all()
        if name in ("neg_inf", "neg_flt_max", "all_nan"):
            assert (warg == -1).all() and (want[0] == -K.FLT_MAX).all() and (g == 0).all()


# ================================================================ RoIAlign
def align_fwd(cuda, feat, rois, AH, AW, scale, name):
    """both layouts: bit for bit against the C oracle, and inside the tolerance rule against the fp64 statement"""
    from scda_amd import native
    want = orc.roi_align_fwd(feat, rois, AH, AW, scale)
    ref = R.roi_align(feat, rois, AH, AW, scale)
    for cm in (False, True):
        out = host(native.roi_align_fwd(dev(feat, cuda), dev(rois, cuda), AH, AW, scale, channel_major=cm))
        if cm:
            out = out.transpose(1, 0, 2, 3)
        same(out, want, f"{name} cmajor={cm}")
        check(f"roi_align_fwd[{name},cmajor={int(cm)}]", out, ref, want)


def align_bwd_forms(cuda, top, rois, shape, AH, AW, scale, monkeypatch):
    """-> {form: gradient}: plane / atomic in the plain layout, and the channel-major layout in whichever form the shape takes and
    in the atomic form"""
    from scda_amd import native
    d_rois = dev(rois, cuda)
    d_top, d_top_cm = dev(top, cuda), dev(top.transpose(1, 0, 2, 3), cuda)
    got = {"default": host(native.roi_align_bwd(d_top, d_rois, shape, AH, AW, scale)),
           "cmajor": host(native.roi_align_bwd(d_top_cm, d_rois, shape, AH, AW, scale, channel_major=True))}
    with monkeypatch.context() as m:
        m.setenv("SCDA_ROI_ALIGN_ATOMIC", "1")
        got["atomic"] = host(native.roi_align_bwd(d_top, d_rois, shape, AH, AW, scale))
        got["cmajor_atomic"] = host(native.roi_align_bwd(d_top_cm, d_rois, shape, AH, AW, scale, channel_major=True))
    return got


def align_bwd_exact(cuda, shape, Rn, AH, AW, name, monkeypatch, seed=0):
    """integer top gradients |g| <= 64 on RoIs whose weights are multiples of 1/64: every product and every partial sum is an exact
    multiple of 1/64 below 2^24 / 64, so every summation order gives the bits of the fp64 statement"""
    B, C, H, W = shape
    rs = np.random.RandomState(AH * 17 + AW + seed)
    rois = K.align_exact_rois(rs, Rn, B, H, W, AH, AW)
    top = rs.randint(-64, 65, (Rn, C, AH, AW)).astype(f32)
    _, g, k, S, wts = R.roi_align(np.zeros(shape, f32), rois, AH, AW, SCALE, top, stats=True)
    assert (wts * 64 == np.round(wts * 64)).all() and S.max() < 2.0 ** 24 / 64 and k.max() > 1
    for form, got in align_bwd_forms(cuda, top, rois, shape, AH, AW, SCALE, monkeypatch).items():
        same(got, g.astype(f32), f"{name} {form}")
    return rois


@pytest.mark.parametrize("grid", [(2, 2), (2, 9), (9, 2), (7, 7), (8, 8), (15, 15), (16, 16), (16, 17)], ids=lambda p: "%dx%d" % p)
def test_roi_align_sample_grids(cuda, grid, monkeypatch):
    """2 x 2 (64 RoIs in flight in the plane backward) ... 15 x 15 (the mask branch: one RoI in flight, 31 threads idle), 16 x 16 = 256
    bins (the plane form's limit), 16 x 17 (atomic form); AH != AW"""
    AH, AW = grid
    rs = np.random.RandomState(AH * 31 + AW)
    shape = (2, 3, 13, 9)
    feat = rs.randn(*shape).astype(f32)
    align_fwd(cuda, feat, K.align_inexact_rois(rs, 33, 2, 13, 9), AH, AW, SCALE, "%dx%d" % grid)
    rois = align_bwd_exact(cuda, shape, 33, AH, AW, "%dx%d" % grid, monkeypatch)
    align_fwd(cuda, feat, rois, AH, AW, SCALE, "%dx%d,exact" % grid)


@pytest.mark.parametrize("shape", [(1, 2, 2, 2), (1, 1, 128, 128), (1, 1, 5, 3277), (3, 2, 6, 7)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_roi_align_planes(cuda, shape, monkeypatch):
    """a 2 x 2 map (every sample in the one cell); 128 x 128 = 16384 pixels = exactly 64 KB (plane form) | 5 x 3277 = 16385 (atomic
    form); three images of which image 1 has no RoI (its gradient stays exactly zero)"""
    B, C, H, W = shape
    rs = np.random.RandomState(H * W)
    feat = rs.randn(*shape).astype(f32)
    Bn = 2 if B == 3 else B
    rois = K.align_inexact_rois(rs, 12, Bn, H, W)
    ex = K.align_exact_rois(rs, 12, Bn, H, W, 7, 7)
    if B == 3:
        rois[:, 0] *= 2; ex[:, 0] *= 2
    align_fwd(cuda, feat, rois, 7, 7, SCALE, "plane %dx%d" % (H, W))
    top = rs.randint(-64, 65, (12, C, 7, 7)).astype(f32)
    _, g = R.roi_align(np.zeros(shape, f32), ex, 7, 7, SCALE, top)
    assert np.abs(g).sum() > 0
    for form, got in align_bwd_forms(cuda, top, ex, shape, 7, 7, SCALE, monkeypatch).items():
        same(got, g.astype(f32), form)
        if B == 3:
            assert (got[1] == 0).all()


@pytest.mark.parametrize("rc", [(1, 1), (3, 5), (5, 3)], ids=lambda p: "R%dC%d" % p)
def test_roi_align_layouts(cuda, rc, monkeypatch):
    """R != C in both orders: a swapped (roi, channel) decode of either layout shows"""
    Rn, C = rc
    rs = np.random.RandomState(Rn * 8 + C)
    shape = (1, C, 6, 7)
    align_fwd(cuda, rs.randn(*shape).astype(f32), K.align_inexact_rois(rs, Rn, 1, 6, 7), 7, 7, SCALE, "R%dC%d" % rc)
    align_bwd_exact(cuda, shape, Rn, 7, 7, "R%dC%d" % rc, monkeypatch)


def test_roi_align_second_sweep(cuda, monkeypatch):
    """75 RoIs x 256 channels x 15 x 15 = 4,320,000 outputs on a 6 x 6 map: more than the 2048 * 8 * 256 = 4,194,304 threads of one
    sweep of the element-wise forms (forward, atomic backward), in both layouts"""
    from scda_amd import native
    Rn, C, A = 75, 256, 15
    shape = (1, C, 6, 6)
    rs = np.random.RandomState(75)
    feat = rs.randint(-8, 9, shape).astype(f32)
    rois = K.align_exact_rois(rs, Rn, 1, 6, 6, A, A)
    top = rs.randint(-64, 65, (Rn, C, A, A)).astype(f32)
    ref, g, k, S, wts = R.roi_align(feat, rois, A, A, SCALE, top, stats=True)       # integer features x weights in 1/64: exact in fp32 too
    assert Rn * C * A * A > 2048 * 8 * 256 and S.max() < 2.0 ** 24 / 64 and (wts * 64 == np.round(wts * 64)).all()
    d_feat, d_rois = dev(feat, cuda), dev(rois, cuda)
    same(host(native.roi_align_fwd(d_feat, d_rois, A, A, SCALE)), ref.astype(f32))
    same(host(native.roi_align_fwd(d_feat, d_rois, A, A, SCALE, channel_major=True)).transpose(1, 0, 2, 3), ref.astype(f32))
    monkeypatch.setenv("SCDA_ROI_ALIGN_ATOMIC", "1")
    same(host(native.roi_align_bwd(dev(top, cuda), d_rois, shape, A, A, SCALE)), g.astype(f32))
    same(host(native.roi_align_bwd(dev(top.transpose(1, 0, 2, 3), cuda), d_rois, shape, A, A, SCALE, channel_major=True)), g.astype(f32))


@pytest.mark.parametrize("A", [2, 3])
def test_roi_align_geometry(cuda, A, monkeypatch):
    """samples exactly on row H - 1 / column W - 1 (hstart = H - 2, ratio 1), one ulp below H (ratio 2 - ulp: the weights leave [0, 1],
    as in the reference), one ulp below 0 (outside) and on -0.0 (inside); roi_w and roi_h clamped to 0; RoIs wholly outside"""
    rs = np.random.RandomState(A)
    shape = (1, 2, 6, 7)
    feat = rs.randn(*shape).astype(f32)
    rois = K.align_geometry_rois(6, 7)
    align_fwd(cuda, feat, rois, A, A, 1.0, "geometry %dx%d" % (A, A))
    want = orc.roi_align_fwd(feat, rois, A, A, 1.0)
    assert (want[3, :, 0, :] == 0).all() and (want[3, :, :, 0] == 0).all() and (want[3, :, 1, 1] != 0).all()    # only row / column 0 outside
    assert (want[6:10] == 0).all() and (want[4, :, 0, 0] != 0).all() and (want[2, :, 0, 0] != 0).all() and (want[2, :, 1:, 1:] == 0).all()
    if A == 2:
        same(want[1, :, 1, 1], feat[0, :, 5, 6])             # the sample on (H - 1, W - 1) is that pixel
    top = K.signed_unit_tops(rs, want.shape)
    _, g, k, S, _ = R.roi_align(feat, rois, A, A, 1.0, top, stats=True)
    for form, got in align_bwd_forms(cuda, top, rois, shape, A, A, 1.0, monkeypatch).items():
        assert (np.abs(got - g) <= (k + 2) * 2.0 ** -24 * S).all(), form


def test_roi_align_nan_coordinate_forward(cuda):
    """a NaN corner fails every `h < 0 || h >= H` test, so the samples count as inside, fminf drops the NaN from the corner index
    (H - 2) and the ratios are NaN: NaN outputs, in-bounds reads.  The same NaN pattern as the oracle's, other RoIs untouched."""
    from scda_amd import native
    feat = np.random.RandomState(4).randn(1, 2, 6, 7).astype(f32)
    rois = np.array([[0, np.nan, 16, 48, 48], [0, 16, 16, 48, np.nan], [0, 16, 16, 48, 48], [0, 16, np.nan, np.nan, 48]], f32)
    want = orc.roi_align_fwd(feat, rois, 3, 3, SCALE)
    for cm in (False, True):
        out = host(native.roi_align_fwd(dev(feat, cuda), dev(rois, cuda), 3, 3, SCALE, channel_major=cm))
        out = out.transpose(1, 0, 2, 3) if cm else out
        same(np.isnan(out), np.isnan(want))
        same(out[2], want[2])
    assert np.isnan(want[0]).all() and not np.isnan(want[2]).any()


@pytest.mark.parametrize("case", ["random_8x8", "random_15x15", "pile_7x7", "large_plane_8x8"])
def test_roi_align_bwd_inexact(cuda, case, monkeypatch):
    """random geometry (and 300 identical zero-size RoIs piled on one cell).  Per gradient pixel, with k contributions of absolute sum S
    (fp64 statement): |kernel - ref64| <= (k + 2) 2^-24 S -- each contribution is rounded once to fp32 (k 2^-24 S in total at most),
    the sum takes k - 1 additions of partial sums <= S and one final add into the output.  Top gradients are drawn from +-[0.5, 1.5],
    so a lost or doubled contribution of weight >= 2^-10 in magnitude (at least 90 % of them, asserted) changes its pixel by >= 2^-11:
    over the bound wherever (k + 2) S < 2^13, which is every pixel but the pile's (k = 14700 there, a bound of about 3: that case checks that
    thousands of additions to one address all arrive, not single losses)."""
    rs = np.random.RandomState(len(case))
    shape, Rn, A, pile = {"random_8x8": ((2, 3, 13, 9), 65, 8, 0), "random_15x15": ((1, 2, 20, 27), 20, 15, 0),
                          "pile_7x7": ((1, 2, 6, 7), 310, 7, 300), "large_plane_8x8": ((1, 1, 5, 3277), 40, 8, 0)}[case]
    B, C, H, W = shape
    rois = K.align_inexact_rois(rs, Rn, B, H, W, pile=pile)
    top = K.signed_unit_tops(rs, (Rn, C, A, A))
    _, g, k, S, wts = R.roi_align(np.zeros(shape, f32), rois, A, A, SCALE, top, stats=True)
    heavy = float((np.abs(wts) >= 2.0 ** -10).mean())       # (a sample between rows H - 1 and H has weights outside [0, 1])
    assert heavy >= 0.9, heavy
    if pile:
        assert k.max() >= 300 * 49
    bound = (k + 2) * 2.0 ** -24 * S
    for form, got in align_bwd_forms(cuda, top, rois, shape, A, A, SCALE, monkeypatch).items():
        err = np.abs(got - g)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"\nEDGE roi_align_bwd[{case},{form}] kmax={int(k.max())} heavy={heavy:.3f} worst_err/bound={worst:.3e} max_err={err.max():.3e}")
        assert (err <= bound).all(), (case, form, worst)


# ================================================================ focal losses
HYPER = [(g, a, w) for g in (0.0, 2.0) for a in (0.0, 0.25, 1.0) for w in (0.0, 0.5, 97.0)]


def focal_all(cuda, rows, C, gamma, alpha, wp):
    from scda_amd import native
    tag = f"rows={rows},C={C},g={gamma:g},a={alpha:g},wp={wp:g}"
    x, t = K.focal_case(rows, C, softmax=False)
    dx, dt = dev(x, cuda), dev(t, cuda)
    for fn in ("focal_sigmoid_fwd", "focal_sigmoid_bwd"):
        got = host(getattr(native, fn)(dx, dt, wp, gamma, alpha, C))
        o32 = getattr(orc, fn)(x, t, wp, gamma, alpha, C)
        assert not np.isnan(got).any(), fn
        check(f"{fn}[{tag}]", got, getattr(R, fn)(x, t, wp, gamma, alpha, C), o32)
        np.testing.assert_allclose(got, o32, atol=1e-6, rtol=1e-5, err_msg=fn)
    x, t = K.focal_case(rows, C, softmax=True)
    dx, dt = dev(x, cuda), dev(t, cuda)
    l, p = native.focal_softmax_fwd(dx, dt, wp, gamma, alpha, C)
    ol, op = orc.focal_softmax_fwd(x, t, wp, gamma, alpha, C)
    rl, rp = R.focal_softmax_fwd(x, t, wp, gamma, alpha, C)
    assert not np.isnan(host(l)).any() and not np.isnan(host(p)).any()
    check(f"focal_softmax_prob[{tag}]", host(p), rp, op)
    check(f"focal_softmax_fwd[{tag}]", host(l), rl, ol)
    np.testing.assert_allclose(host(p), op, atol=1e-6)
    np.testing.assert_allclose(host(l), ol, atol=1e-6, rtol=1e-5)
    # the backward on the ORACLE's probabilities: kernel, oracle and fp64 formula then see one input
    g = host(native.focal_softmax_bwd(dx, dt, dev(op, cuda), wp, gamma, alpha, C))
    og = orc.focal_softmax_bwd(x, t, op, wp, gamma, alpha, C)
    rg = R.focal_softmax_bwd(op, t, wp, gamma, alpha, C)
    assert not np.isnan(g).any()
    ok = np.isfinite(rg)
    assert gamma < 1 or ok.all()
    check(f"focal_softmax_bwd[{tag}]", g, rg, og, ok=None if ok.all() else ok)
    np.testing.assert_allclose(g[ok], og[ok], atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("gamma,alpha,wp", HYPER, ids=lambda v: "%g" % v)
def test_focal_hyper_parameters(cuda, gamma, alpha, wp):
    """logits 0, -0.0, +-17, +-88, +-100 on every target value (sigmoid: -1, 0, every class, C, C + 1; softmax: -1 .. C - 1), tied
    rows and rows of -100, at rows = 257 (one workgroup and one thread) and C = 8"""
    focal_all(cuda, 257, 8, gamma, alpha, wp)


@pytest.mark.parametrize("rows,C", [(1, 8), (255, 8), (65537, 8), (257, 1), (257, 2), (257, 81)], ids=lambda v: "%d" % v)
def test_focal_sizes(cuda, rows, C):
    """65537 rows of 8: one element-wise sweep of 2048 * 256 = 524288 threads plus a tail of 8; one class (a softmax that is exactly
    1: the weight's 0 * inf corner) ... 81"""
    focal_all(cuda, rows, C, 2.0, 0.25, 97.0)
    focal_all(cuda, rows, C, 0.0, 1.0, 0.5)


def test_focal_fractional_gamma(cuda):
    """gamma = 0.5: (1 - p)^(gamma - 1) overflows in the fp64 formula where 1 - p is tiny; compared where it is finite, no NaN anywhere"""
    focal_all(cuda, 257, 8, 0.5, 0.25, 97.0)
    focal_all(cuda, 257, 1, 0.5, 0.25, 0.5)


# ================================================================ overlaps
@pytest.mark.parametrize("n1,n2", [(1, 1), (512, 1024), (3, 174763), (174763, 3), (1, 300), (300, 1)], ids=lambda v: "%d" % v)
@pytest.mark.parametrize("sz", [4, 5])
def test_overlaps_bit_exact(cuda, n1, n2, sz):
    """n1 * n2 = 1, 524288 (one sweep of the launch exactly) and 524289 (a second sweep of one element); N = 1, K = 1; boxes of 4 and 5
    columns; touching boxes (iw == 0), zero-area and inverted boxes, unions below 1 (the clamp)"""
    from scda_amd import native
    a, b = K.overlap_case(n1, n2, sz)
    want = R.iou_overlaps(a, b)
    same(host(native.iou_overlaps(dev(a, cuda), dev(b, cuda))), want)
    if sz == 4:
        same(host(native.bbox_overlaps(dev(a, cuda), dev(b, cuda))), R.bbox_overlaps(a, b))
    if n1 * n2 > 100:
        assert (want == 0).any() and (want > 0).any()
