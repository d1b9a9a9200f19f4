"""tests/conv_refs.py against torch itself, on the CPU: the Winograd restatement equals the convolution, its magnitude sum dominates the
direct one, the stacked form is the batched convolution, every integer case of tests/test_conv_edges_gpu.py is exact in float32 in
the restatements (so a kernel that misses one is wrong, not the inputs), and every case takes the kernel form its name says."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R


def _autograd(x, w, b, dy):
    x = x.double().requires_grad_(); w = w.double().requires_grad_(); b = b.double().requires_grad_()
    y = F.conv2d(x, w, b, padding=1)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("shape", [(2, 8, 4, 6, 5), (1, 7, 2, 2, 8), (3, 16, 6, 4, 9), (1, 3, 8, 34, 1)])       # B, Cin, H, W, Cout
def test_winograd_restatement_is_the_convolution(shape):
    B, Cin, H, W, Cout = shape
    g = R.gen(sum(shape))
    x = torch.randn(B, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g); b = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    y, dx, dw, db = _autograd(x, w, b, dy)
    yw, Sy = R.wino_fwd(x, w, b)
    dxw, Sdx = R.wino_dgrad(dy, w)
    (dww, dbw), (Sdw, Sdb) = R.wino_wgrad(dy, x)
    for got, want, Sw in ((yw, y, Sy), (dxw, dx, Sdx), (dww, dw, Sdw), (dbw, db, Sdb)):
        assert got.shape == want.shape
        assert ((got - want).abs() <= 1e-12 * Sw).all()
    # the direct restatements, likewise, and S_w >= S everywhere
    yd, S = R.conv_fwd(x, w, b, 1, 1)
    dxd, Sd = R.conv_dgrad(dy, w, x.shape, 1, 1)
    (dwd, dbd), (Swd, Sbd) = R.conv_wgrad(dy, x, w.shape, 1, 1)
    for got, want, Sdir, Sw in ((yd, y, S, Sy), (dxd, dx, Sd, Sdx), (dwd, dw, Swd, Sdw), (dbd, db, Sbd, Sdb)):
        assert ((got - want).abs() <= 1e-12 * Sdir).all()
        assert (Sw >= Sdir * (1 - 1e-14)).all() and (Sdir >= want.abs() * (1 - 1e-14)).all()


def test_masks_activations_and_accumulation():
    g = R.gen(3)
    x = torch.randn(2, 8, 4, 4, generator=g); w = torch.randn(8, 8, 3, 3, generator=g); b = torch.randn(8, generator=g)
    dy = torch.randn(2, 8, 4, 4, generator=g); prev = torch.randn(8, 8, 3, 3, generator=g); pdb = torch.randn(8, generator=g)
    want = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.25)
    for fn in (lambda: R.conv_fwd(x, w, b, 1, 1, R.ACT_LEAKY, 0.25), lambda: R.wino_fwd(x, w, b, R.ACT_LEAKY, 0.25)):
        assert torch.allclose(fn()[0], want, rtol=0, atol=1e-12)
    m = torch.where(x > 0, 1.0, 0.5).double()
    want = _autograd(x, w, b, dy)[1] * m
    for fn in (lambda: R.conv_dgrad(dy, w, x.shape, 1, 1, x, 0.5), lambda: R.wino_dgrad(dy, w, x, 0.5)):
        assert torch.allclose(fn()[0], want, rtol=0, atol=1e-12)
    _, _, dw, db = _autograd(x, w, b, dy)
    for fn in (lambda: R.conv_wgrad(dy, x, w.shape, 1, 1, prev, pdb), lambda: R.wino_wgrad(dy, x, prev, pdb)):
        (gw, gb), (Sw, Sb) = fn()
        assert torch.allclose(gw, dw + prev.double(), rtol=0, atol=1e-12) and torch.allclose(gb, db + pdb.double(), rtol=0, atol=1e-12)
        assert (Sw >= prev.abs().double()).all() and (Sb >= pdb.abs().double()).all()


@pytest.mark.parametrize("stride,pad,k,hw", [(2, 1, 3, (5, 6)), (2, 1, 3, (4, 4)), (2, 0, 1, (5, 7)), (1, 0, 3, (3, 3)), (2, 3, 7, (4, 4))])
def test_strided_direct_restatements_against_autograd(stride, pad, k, hw):
    g = R.gen(stride + pad + k)
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(4, 3, k, k, generator=g, dtype=torch.float64).requires_grad_()
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    assert torch.allclose(R.conv_dgrad(dy, w.detach(), x.shape, stride, pad)[0], x.grad, rtol=0, atol=1e-12)
    assert torch.allclose(R.conv_wgrad(dy, x.detach(), w.shape, stride, pad)[0][0], w.grad, rtol=0, atol=1e-12)


@pytest.mark.parametrize("maps", [1, 3, 4, 5])
def test_stacked_form_is_the_batched_convolution(maps):
    g = R.gen(maps)
    xb = torch.randn(maps, 8, 7, 7, generator=g); w = torch.randn(16, 8, 3, 3, generator=g); b = torch.randn(16, generator=g)
    dyb = torch.randn(maps, 16, 7, 7, generator=g)
    y, dx, dw, db = _autograd(xb, w, b, dyb)
    xs, dys = R.stack(xb), R.stack(dyb)
    assert xs.shape == (1, 8, maps * 7, 7) and torch.equal(R.unstack(xs), xb)
    for fwd, dgrad, wgrad in ((R.stacked_fwd, R.stacked_dgrad, lambda a, c: R.stacked_wgrad(a, c, w.shape)),
                              (R.wino_stacked_fwd, R.wino_stacked_dgrad, R.wino_stacked_wgrad)):
        assert torch.allclose(R.unstack(fwd(xs, w, b)[0]), y, rtol=0, atol=1e-11)
        assert torch.allclose(R.unstack(dgrad(dys, w)[0]), dx, rtol=0, atol=1e-11)
        (gw, gb), _ = wgrad(dys, xs)
        assert torch.allclose(gw, dw, rtol=0, atol=1e-11) and torch.allclose(gb, db, rtol=0, atol=1e-11)


def test_gemm_layouts():
    g = R.gen(5)
    a = torch.randn(5, 7, generator=g); b = torch.randn(3, 7, generator=g); bias = torch.randn(3, generator=g); prev = torch.randn(5, 3, generator=g)
    want = a.double() @ b.double().t()
    for ta, tb in R.LAYOUTS:
        A = a.t().contiguous() if ta else a
        Bm = b.t().contiguous() if tb else b
        c, S = R.gemm(A, Bm, ta, tb)
        assert torch.allclose(c, want, rtol=0, atol=1e-13) and (S >= c.abs() * (1 - 1e-14)).all()
    c, S = R.gemm(a, b, bias=bias, act=R.ACT_RELU, prev=prev)
    assert torch.allclose(c, torch.relu(want + bias.double()) + prev.double(), rtol=0, atol=1e-13)


# ---------------------------------------------------------------- the integer cases are exact in float32
def _exact(f):
    v64, S = f(torch.float64)
    v32, _ = f(torch.float32)
    flat = lambda t: list(t) if isinstance(t, tuple) else [t]
    for a, b, s in zip(flat(v64), flat(v32), flat(S)):
        assert 4 * s.max().item() < 2 ** 24
        assert torch.equal(a.float(), b) and torch.equal(a.float().double(), a)


@pytest.mark.parametrize("case", R.DIRECT_CASES, ids=[c[0] for c in R.DIRECT_CASES])
def test_integer_direct_cases_are_exact_in_float32(case):
    name, B, Cin, H, W, Cout, k, s, p, rp, force, dirs = case
    d = R.direct_data(case, "int")
    for f in R.direct_refs(case, d).values():
        _exact(f)


@pytest.mark.parametrize("case", R.WINO_CASES, ids=[c[0] for c in R.WINO_CASES])
def test_integer_winograd_cases_are_exact_in_float32(case):
    d = R.wino_data(case, "int")
    for f in R.wino_refs(case, d).values():
        _exact(f)
    for f in R.wino_refs(case, d, direct=True).values():       # ... and in the direct restatement of the same layer
        _exact(f)


@pytest.mark.parametrize("case", R.GEMM_CASES, ids=[c[0] for c in R.GEMM_CASES])
def test_integer_gemm_cases_are_exact_in_float32(case):
    for ta, tb in R.LAYOUTS:
        d = R.gemm_data(case, ta, tb, "int")
        for f in R.gemm_refs(d, ta, tb).values():
            _exact(f)


# ---------------------------------------------------------------- every case takes the form its name says (no GPU: launch_plan.h)
def test_direct_cases_take_their_forms(monkeypatch):
    from scda_amd import native
    monkeypatch.setenv("SCDA_WINOGRAD", "0")
    fams = {}
    for case in R.DIRECT_CASES:
        name, B, Cin, H, W, Cout, k, s, p, rp, force, dirs = case
        assert native._route(0, B, Cin, H, W, Cout, k, k, s, p, rp)[0] == 0
        if force and dirs == "w":
            with R.plan_env(monkeypatch, force, name):
                for kind, al in (("wgrad", True), ("wgrad_bias", True), ("wgrad", False)):
                    plan = native.plan_conv(kind, B, Cin, H, W, Cout, k, s, p, rp, aligned=al)
                    assert (plan["bm"], plan["bn"], plan["splits"]) == force, (name, kind, plan)
        with R.plan_env(monkeypatch, force, name):
            for d in dirs.replace("w", ""):
                plan = native.plan_conv({"f": "fwd", "d": "dgrad"}[d], B, Cin, H, W, Cout, k, s, p, rp)
                if force:
                    assert (plan["bm"], plan["bn"], plan["splits"]) == force, (name, d, plan)
                fams[name, d] = (plan["family"], plan["parity"])
        if "w" in dirs:
            fams[name, "w"] = tuple(native.plan_conv("wgrad", B, Cin, H, W, Cout, k, s, p, rp, aligned=a)[key] for a in (True, False)
                                    for key in ("family", "bm"))
    # both gather families, the small-Cin kernel, parity classes; LDS-DMA and register-staged weight gradients, the 32-row tile
    assert fams["map1x1", "f"] == (1, 0) and fams["mapHx1", "f"] == (0, 0) and fams["small_cin", "f"] == (3, 0) and fams["stem7x7", "f"] == (0, 0)
    assert fams["s2_parity", "d"] == (1, 1) and fams["s2_odd", "d"] == (1, 0) and fams["s2_parity_split", "d"] == (1, 1)
    assert fams["wgrad_lds_dma", "w"] == (1, 64, 0, 64) and fams["wgrad_lds_dma_tile32", "w"] == (1, 32, 0, 64)
    assert fams["wgrad_lds_dma_cout1", "w"] == (1, 32, 0, 64) and fams["wgrad_lds_dma_128rows", "w"] == (1, 128, 0, 128)
    assert fams["wgrad_lds_dma_256rows", "w"] == (1, 256, 0, 128) and fams["wgrad_staged_128rows", "w"] == (0, 128, 0, 128)
    assert fams["wgrad_8_splits", "w"][0] == 1 and fams["wgrad_32_splits", "w"][0] == 1
    assert fams["wgrad_vec4", "w"][0] == 0 and fams["wgrad_27_pixels", "w"][0] == 0 and fams["wgrad_one_partial_slab", "w"][0] == 0
    for name in ("stack1", "stack3", "stack4", "stack5"):
        assert fams[name, "f"][0] == (0 if name == "stack5" else 1)


def test_winograd_and_gemm_cases_take_their_forms(monkeypatch):
    from scda_amd import native
    for case in R.WINO_CASES:
        name, B, C, H, W, M, maps, env, dirs, expect = case
        with R.plan_env(monkeypatch, None, name, env):
            if "f" in dirs:
                p = native.plan_wino("fwd", B, C, H, W, M, 7 if maps else 0)
                assert (bool(p["persist"]), p["gm"]) == expect[:2] and expect[2] in (None, p["splits"]), (name, p)
            if "w" in dirs and not maps:
                assert native.plan_wino("wgrad_bias", B, C, H, W, M)["splits"] == expect, name
    for case in R.GEMM_CASES:
        name, M, N, K, force, env = case
        with R.plan_env(monkeypatch, force, name, env):
            fams = []
            for ta, tb in R.LAYOUTS:
                if name == "tile256x128" and ta and tb:
                    continue
                p = native.plan_gemm(M, N, K, M if ta else K, N if tb else K, ta, tb)
                if force:
                    assert (p["bm"], p["bn"], p["splits"]) == force, (name, p)
                assert native.plan_gemm(M, N, K, M if ta else K, N if tb else K, ta, tb, aligned=False)["family"] == 0
                fams.append(p["family"])
            if name.startswith("x9"):
                assert 2 in fams, (name, fams)
