"""The convolution, Winograd and GEMM kernels (scda_amd/csrc/conv_gemm.hip, conv_wino.hip) element-wise against the fp64 restatements of
tests/conv_refs.py (checked on the CPU by tests/test_conv_refs.py), at the smallest shapes at which each kernel form exists.

A. Componentwise rule.  With S the magnitude sum of an output element (sum |a||b| + |bias| + |previous out|; S_w of the transform
   chain for a launch that ran a Winograd kernel), e_i = |got_i - ref64_i| / S_i, E_kernel = max e_i and E32 the same figure of an fp32
   CPU evaluation that is not the code under test (torch's conv2d / conv_transpose2d / conv2d_weight / matmul; the Winograd
   restatement in float32):
       E_kernel <= max(FACTOR * E32, 4 * 2^-23)            and the bound is below the worst case (K + 8) * 2^-24 of a K-term chain.
   Where S_i = 0 the output is +-0.  FACTOR per family: see FACTOR below and profiles/conv_edges.txt.
B. Integer operands (4 max S < 2^24, asserted): every partial sum of any order, split or transform is exact -- torch.equal.
C. Offset views: contiguous operands 4 bytes off a 16-byte boundary, one at a time and all at once.
D. Guard bands: inputs inside NaN, accumulated outputs inside a sentinel pattern that must come back unchanged.
E. One +inf in an operand reaches its receptive field only.
Every launch proves its form with native.last_plan() / wino_last_order() / wino_last_persistent() against the decision
launch_plan.h gives for the case (test_conv_refs.py pins those decisions on the CPU); a form not taken fails.
Each comparison prints `EDGE <case> <form> E32=... kernel=... bound=...` (pytest -s)."""
import pytest
import torch

import conv_refs as R

pytestmark = pytest.mark.gpu

ULP4 = 4.0 * 2.0 ** -23
# E_kernel / E32 allowed per family (rule A).  4 = a different summation order, the rule of tests/test_nn_ops_edges_gpu.py.
FACTOR = {"direct": 4.0, "wino": 4.0, "gemm": 4.0, "x9": 4.0}
GUARD = 4096                       # floats of guard band on each side
SENTINEL = 0x7FC5A5A5              # (a NaN payload: an output that picked one up is not finite either)
KINDS = ["gauss", "relu", "mean100"]


def flat(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault(cuda):
    """a device fault is sticky: nothing more is launched behind one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault, stopping the run: %s" % e, returncode=3)


# ---------------------------------------------------------------- placements
class Banded:
    """tensors as views inside larger buffers: inputs in NaN, outputs in SENTINEL words"""
    def __init__(self):
        self.outs = []

    def inp(self, t, device):
        buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=device)
        v = buf[GUARD:GUARD + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def out(self, t, device):
        buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)
        v = buf[GUARD:GUARD + t.numel()].view(t.shape)
        v.copy_(t)
        self.outs.append((buf, t.numel()))
        return v

    def check(self):
        assert self.outs
        for buf, n in self.outs:
            w = buf.view(torch.int32).cpu()
            assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all(), "a store left the output tensor"


def place(data, device, offset=(), banded=None):
    """operands on the device: names in `offset` as offset views, with `banded` every input in a NaN band and every accumulated output
    (prev, prev_db) in a sentinel band"""
    T = {}
    for k, t in data.items():
        if banded is not None:
            T[k] = banded.out(t, device) if k.startswith("prev") else banded.inp(t, device)
        elif k in offset or offset == "all":
            T[k] = R.offset_view(t, device)
        else:
            T[k] = t.to(device)
    return T


def aligned(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


# ---------------------------------------------------------------- the two checks
def check_rule_a(label, form, got, ref_f, K, factor):
    v64, S = ref_f(torch.float64)
    v32, _ = ref_f(torch.float32)
    for i, (g, r, s, t) in enumerate(zip(flat(got), flat(v64), flat(S), flat(v32))):
        g = g.detach().cpu().double()
        assert g.shape == r.shape, (label, g.shape, r.shape)
        assert torch.isfinite(r).all() and torch.isfinite(g).all(), label
        zero = s == 0
        assert (g[zero] == 0).all(), "%s: S = 0 but the output is not +-0" % label
        sd = torch.where(zero, torch.ones_like(s), s)
        e32 = ((t.double() - r).abs() / sd).max().item()
        err = ((g - r).abs() / sd).max().item()
        bound = max(factor * e32, ULP4)
        print("\nEDGE %s[%d] %s E32=%.3e kernel=%.3e bound=%.3e K=%d" % (label, i, form, e32, err, bound, K))
        assert bound < (K + 8) * 2.0 ** -24, "%s: the bound %.3e says nothing for a chain of %d terms" % (label, bound, K)
        assert err <= bound, "%s %s: kernel error %.3e of S over %.3e (E32 %.3e)" % (label, form, err, bound, e32)


def check_exact(label, got, ref_f):
    v64, S = ref_f(torch.float64)
    for i, (g, r, s) in enumerate(zip(flat(got), flat(v64), flat(S))):
        assert 4 * s.max().item() < 2 ** 24, label
        g = g.detach().cpu()
        assert torch.isfinite(g).all(), label
        want = r.float()
        if not torch.equal(g, want):
            bad = (g != want).nonzero()
            raise AssertionError("%s[%d]: %d of %d elements differ from the exact result, first at %s: got %r want %r"
                                 % (label, i, len(bad), g.numel(), bad[0].tolist(), g[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


# ---------------------------------------------------------------- direct family
def direct_run(native, case, T, op):
    """one operation of a DIRECT_CASES entry on the device -> (outputs, form); the launch decision is checked against launch_plan.h"""
    name, B, Cin, H, W, Cout, k, s, p, rp, force, dirs = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1

    def proved(direction, al=True):
        plan = native.plan_conv(direction, B, Cin, H, W, Cout, k, s, p, rp, aligned=al)
        lp = native.last_plan()
        assert lp[:3] == (plan["bm"], plan["bn"], plan["splits"]) and (lp[3] is True) == (plan["family"] == 1), (name, op, lp, plan)
        return "%s:fam%d,%dx%d,s%d%s" % (direction, plan["family"], plan["bm"], plan["bn"], plan["splits"], ",parity" if plan["parity"] else "")

    if op.startswith("fwd"):
        bias, act, slope = {"fwd": (None, 0, 0.0), "fwd_relu": (T["bias"], 1, 0.0), "fwd_leaky": (T["bias"], 2, 0.25)}[op]
        with R.plan_env(pytest.MonkeyPatch, force, name):
            y = native.conv2d_fwd(T["x"], T["w"], bias, s, p, act, slope, row_period=rp)
            form = proved("fwd")
            if force:
                assert native.last_plan()[:3] == force, (name, native.last_plan())
        return y, form
    if op.startswith("dgrad"):
        src, slope = (T["src"], 0.5) if op == "dgrad_mask" else (None, 0.0)
        with R.plan_env(pytest.MonkeyPatch, force, name):
            dx = native.conv2d_dgrad(T["dy"], T["w"], (B, Cin, H, W), s, p, act_src=src, act_slope=slope, row_period=rp)
            if src is None and Cin <= 4:
                return dx, "dgrad:small_cin"        # (conv_dgrad_small_cin_kernel: no tiles, no plan)
            form = proved("dgrad")
            if force:
                assert native.last_plan()[:3] == force, (name, native.last_plan())
        return dx, form
    out, db_out = (T["prev"], T["prev_db"]) if op == "wgrad_acc" else (None, None)
    with R.plan_env(pytest.MonkeyPatch, force if dirs == "w" else None, name):
        dw, db = native.conv2d_wgrad_bias(T["dy"], T["x"], (Cout, Cin, k, k), s, p, out=out, db_out=db_out, row_period=rp)
        fusable = (OH * OW) % 16 == 0 and aligned(T["dy"])
        form = proved("wgrad_bias" if fusable else "wgrad", aligned(T["dy"]))
        if force and dirs == "w":
            assert native.last_plan()[:3] == force, (name, native.last_plan())
    if not aligned(T["dy"]):
        assert native.last_plan()[3] is False            # the register-staged kernel ran
    return (dw, db), form


def direct_K(case, op):
    name, B, Cin, H, W, Cout, k, s, p = case[:9]
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return Cin * k * k + 1 if op.startswith("fwd") else Cout * k * k if op.startswith("dgrad") else B * OH * OW + 1


DIRECT_OPERANDS = {"fwd": ("x", "w"), "fwd_relu": ("x", "w", "bias"), "fwd_leaky": ("x", "w", "bias"), "dgrad": ("dy", "w"),
                   "dgrad_mask": ("dy", "w", "src"), "wgrad": ("dy", "x"), "wgrad_acc": ("dy", "x", "prev", "prev_db")}


@pytest.fixture
def direct(monkeypatch):
    monkeypatch.setenv("SCDA_WINOGRAD", "0")
    from scda_amd import native
    return native


IDS_D = [c[0] for c in R.DIRECT_CASES]


@pytest.mark.parametrize("case", R.DIRECT_CASES, ids=IDS_D)
def test_direct_componentwise(cuda, direct, case):
    for kind in KINDS:
        data = R.direct_data(case, kind, seed=1)
        T = place(data, cuda)
        for op, ref_f in R.direct_refs(case, data).items():
            got, form = direct_run(direct, case, T, op)
            check_rule_a("direct/%s/%s/%s" % (case[0], op, kind), form, got, ref_f, direct_K(case, op), FACTOR["direct"])


@pytest.mark.parametrize("case", R.DIRECT_CASES, ids=IDS_D)
def test_direct_integer_exact_in_guard_bands(cuda, direct, case):
    """B and D: integer operands, plain and then every input inside NaN and every accumulated output inside sentinel words"""
    data = R.direct_data(case, "int")
    refs = R.direct_refs(case, data)
    for banded in (None, Banded()):
        for op, ref_f in refs.items():
            T = place(data, cuda, banded=banded)
            got, form = direct_run(direct, case, T, op)
            check_exact("direct/%s/%s/%s %s" % (case[0], op, "banded" if banded else "plain", form), got, ref_f)
        if banded is not None and "w" in case[11]:
            banded.check()


OFFSET_DIRECT = [c for c in R.DIRECT_CASES if not c[0].startswith("seam") or c[0] in ("seam64_n64_s2", "seam128_n129_s2", "seam256_n256_s2")]


@pytest.mark.parametrize("case", OFFSET_DIRECT, ids=[c[0] for c in OFFSET_DIRECT])
def test_direct_offset_views(cuda, direct, case):
    """C: one operand at a time 4 bytes off a 16-byte boundary, then all of them; the form that ran is checked inside direct_run (an
    unaligned dy takes the register-staged weight gradient and the separate bias gradient, an unaligned out / act_src the scalar
    reduce; x and the packed weights are read dword-wise by every kernel), then rules B and A"""
    for kind in ("int", "gauss"):
        data = R.direct_data(case, kind, seed=2)
        for op, ref_f in R.direct_refs(case, data).items():
            for which in [(n,) for n in DIRECT_OPERANDS[op]] + ["all"]:
                T = place(data, cuda, offset=which)
                got, form = direct_run(direct, case, T, op)
                label = "direct/%s/%s/offset %s/%s" % (case[0], op, "+".join(which) if which != "all" else "all", kind)
                if kind == "int":
                    check_exact(label + " " + form, got, ref_f)
                else:
                    check_rule_a(label, form, got, ref_f, direct_K(case, op), FACTOR["direct"])


# ---------------------------------------------------------------- Winograd
def wino_run(native, case, T, op):
    name, B, C, H, W, M, maps, env, dirs, expect = case
    rp = 7 if maps else 0
    with R.plan_env(pytest.MonkeyPatch, None, name, env):
        if op.startswith("wgrad"):
            out, db_out = (T["prev"], T["prev_db"]) if op == "wgrad_acc" else (None, None)
            dw, db = native.conv2d_wino_wgrad(T["dy"], T["x"], (M, C, 3, 3), out=out, db_out=db_out, want_bias=True, row_period=rp)
            plan = native.plan_wino("wgrad_bias", B, C, H, W, M, rp)
            order = native.wino_last_order()[1]
            assert order == (plan["splits"], plan["order"]), (name, order, plan)
            if not maps:
                assert order[0] == expect, (name, order)
            return (dw, db), "wino_wgrad:s%d,o%d" % order
        dgrad = op.startswith("dgrad")
        u = native.conv2d_wino_pack(T["w_d" if dgrad else "w_f"], dgrad)
        if dgrad:
            src, slope = (T["src"], 0.5) if op == "dgrad_mask" else (None, 0.0)
            y = native.conv2d_wino(T["x"], u, None, M, 0, 0.0, src, slope, for_dgrad=True, row_period=rp)
            plan = native.plan_wino("dgrad_mask" if src is not None else "dgrad", B, M, H, W, C, rp)
        else:
            act, slope = (1, 0.0) if op == "fwd_relu" else (2, 0.25)
            y = native.conv2d_wino(T["x"], u, T["bias"], M, act, slope, row_period=rp)
            plan = native.plan_wino("fwd", B, C, H, W, M, rp)
        order, persistent = native.wino_last_order()[0], native.wino_last_persistent()
        assert order == (plan["mb"], bool(plan["pixel_major"]), plan["gm"], plan["splits"]) and persistent == bool(plan["persist"]), (name, order, plan)
        assert (persistent, order[2]) == expect[:2] and expect[2] in (None, order[3]), (name, op, order, persistent)
        return y, "wino:mb%d,gm%d,s%d%s" % (order[0], order[2], order[3], ",persistent" if persistent else "")


def wino_K(case, op):
    name, B, C, H, W, M = case[:6]
    return 4 * B * H * W + 1 if op.startswith("wgrad") else 9 * C + 8


WINO_OPERANDS = {"fwd_relu": ("x", "w_f", "bias"), "fwd_leaky": ("x", "w_f", "bias"), "dgrad": ("x", "w_d"), "dgrad_mask": ("x", "w_d", "src"),
                 "wgrad": ("dy", "x"), "wgrad_acc": ("dy", "x", "prev", "prev_db")}
IDS_W = [c[0] for c in R.WINO_CASES]


@pytest.fixture
def native_mod():
    from scda_amd import native
    return native


@pytest.mark.parametrize("case", R.WINO_CASES, ids=IDS_W)
def test_wino_componentwise(cuda, native_mod, case):
    for kind in KINDS:
        data = R.wino_data(case, kind, seed=1)
        for op, ref_f in R.wino_refs(case, data).items():
            got, form = wino_run(native_mod, case, place(data, cuda), op)
            check_rule_a("wino/%s/%s/%s" % (case[0], op, kind), form, got, ref_f, wino_K(case, op), FACTOR["wino"])


@pytest.mark.parametrize("case", R.WINO_CASES, ids=IDS_W)
def test_wino_integer_exact_in_guard_bands(cuda, native_mod, case):
    data = R.wino_data(case, "int")
    refs = R.wino_refs(case, data)
    for banded in (None, Banded()):
        for op, ref_f in refs.items():
            got, form = wino_run(native_mod, case, place(data, cuda, banded=banded), op)
            check_exact("wino/%s/%s/%s %s" % (case[0], op, "banded" if banded else "plain", form), got, ref_f)
        if banded is not None and "w" in case[8]:
            banded.check()


@pytest.mark.parametrize("case", R.WINO_CASES, ids=IDS_W)
def test_wino_offset_views_give_the_aligned_bits(cuda, native_mod, case):
    """C: no branch of conv_wino.hip depends on alignment (dword LDS-DMA of the patches; the 8-byte mask loads and paired stores and the
    reduce kernels' 16-byte forms are what an offset operand meets): the result equals the aligned call bit for bit, and is exact"""
    data = R.wino_data(case, "int", seed=2)
    for op, ref_f in R.wino_refs(case, data).items():
        base, _ = wino_run(native_mod, case, place(data, cuda), op)
        for which in [(n,) for n in WINO_OPERANDS[op]] + ["all"]:
            got, form = wino_run(native_mod, case, place(data, cuda, offset=which), op)
            for a, b in zip(flat(got), flat(base)):
                assert torch.equal(bits(a), bits(b)), (case[0], op, which)
            check_exact("wino/%s/%s/offset %s %s" % (case[0], op, which, form), got, ref_f)
    data = R.wino_data(case, "gauss", seed=3)
    for op in R.wino_refs(case, data):
        base, _ = wino_run(native_mod, case, place(data, cuda), op)
        got, _ = wino_run(native_mod, case, place(data, cuda, offset="all"), op)
        for a, b in zip(flat(got), flat(base)):
            assert torch.equal(bits(a), bits(b)), (case[0], op)


# ---------------------------------------------------------------- dense GEMM
def gemm_run(native, case, ta, tb, T, op):
    name, M, N, K, force, env = case
    lda, ldb = (M if ta else K), (N if tb else K)
    kw = {"plain": {}, "bias_relu": dict(bias=T["bias"], bias_on_n=True, act=1), "bias_m_leaky": dict(bias=T["bias_m"], bias_on_n=False, act=2, slope=0.25),
          "accumulate": dict(out=T["prev"], accumulate=True)}[op]
    with R.plan_env(pytest.MonkeyPatch, force, name, env):
        c = native.gemm(T["a"], T["b"], M, N, K, lda, ldb, ta, tb, **kw)
        al = aligned(T["a"], T["b"])
        plan = native.plan_gemm(M, N, K, lda, ldb, ta, tb, aligned=al)
        lp = native.last_plan()
        fam = 2 if lp[3] == 2 else 1 if lp[3] else 0
        assert lp[:2] == (plan["bm"], plan["bn"]) and fam == plan["family"] and lp[2] == (-1 if plan["x9_stream"] else plan["splits"]), (name, lp, plan)
        if force and (al or force[0] <= 128):      # (the 256-row tile exists on the direct-to-LDS kernel only)
            assert lp[:3] == force
        if not al:
            assert fam == 0          # unaligned operands: the register-staged kernel
    return c, "gemm:fam%d,%dx%d,s%d" % (fam, lp[0], lp[1], lp[2])


# (the 256-row tile has no [K][M] x [K][N] form: launch_plan.h decide_gemm)
GEMM_PARAMS = [(c, ta, tb) for c in R.GEMM_CASES for ta, tb in R.LAYOUTS if not (c[0] == "tile256x128" and ta and tb)]
IDS_G = ["%s-%s%s" % (c[0], "T" if ta else "N", "T" if tb else "N") for c, ta, tb in GEMM_PARAMS]


@pytest.mark.parametrize("case,ta,tb", GEMM_PARAMS, ids=IDS_G)
def test_gemm_componentwise_exact_offset_banded(cuda, native_mod, case, ta, tb):
    """A (three input kinds), B + D (integers, plain and in guard bands) and C (A / B / out offset, one at a time and together)"""
    K = case[3] + 1
    for kind in KINDS:
        data = R.gemm_data(case, ta, tb, kind, seed=1)
        for op, ref_f in R.gemm_refs(data, ta, tb).items():
            got, form = gemm_run(native_mod, case, ta, tb, place(data, cuda), op)
            check_rule_a("gemm/%s/%s/%s" % (case[0], op, kind), form, got, ref_f, K, FACTOR["x9" if "fam2" in form else "gemm"])
    data = R.gemm_data(case, ta, tb, "int")
    refs = R.gemm_refs(data, ta, tb)
    banded = Banded()
    for op, ref_f in refs.items():
        for how in ("plain", "banded", ("a",), ("b",), ("prev",), "all"):
            if how == ("prev",) and op != "accumulate":
                continue
            T = place(data, cuda, banded=banded) if how == "banded" else place(data, cuda, offset=() if how == "plain" else how)
            got, form = gemm_run(native_mod, case, ta, tb, T, op)
            check_exact("gemm/%s/%s/%s %s" % (case[0], op, how, form), got, ref_f)
    banded.check()
    data = R.gemm_data(case, ta, tb, "gauss", seed=2)
    for op, ref_f in R.gemm_refs(data, ta, tb).items():
        got, form = gemm_run(native_mod, case, ta, tb, place(data, cuda, offset="all"), op)
        check_rule_a("gemm/%s/%s/offset all" % (case[0], op), form, got, ref_f, K, FACTOR["gemm"])


# ---------------------------------------------------------------- E: locality of a planted inf
def _case(cases, name):
    return next(c for c in cases if c[0] == name)


def _same_outside(got, base, touched, label):
    g, b = got.detach().cpu(), base.detach().cpu()
    assert torch.equal(bits(g)[~touched], bits(b)[~touched]), "%s: an output outside the receptive field changed" % label
    if touched.any():          # (a stride-2 1x1 layer never reads the odd pixels)
        assert not torch.isfinite(g[touched]).all(), "%s: the planted inf reached nothing" % label


@pytest.mark.parametrize("name", ["seam64_n65_s1", "seam128_n128_s2", "s2_parity", "stack3", "mapHx1", "k1_stride2"])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_direct_planted_inf_stays_in_its_window(cuda, direct, name, where):
    case = _case(R.DIRECT_CASES, name)
    _, B, Cin, H, W, Cout, k, s, p, rp, force, dirs = case
    data = R.direct_data(case, "gauss", seed=5)
    base, _ = direct_run(direct, case, place(data, cuda), "fwd_leaky")
    n, c, y, x = (B - 1, Cin // 2, H // 2, W // 2) if where == "interior" else (0, 0, H - 1, W - 1)
    data["x"][n, c, y, x] = float("inf")
    got, form = direct_run(direct, case, place(data, cuda), "fwd_leaky")
    touched = torch.zeros(base.shape, dtype=torch.bool)
    for oy in range(base.shape[2]):
        for ox in range(base.shape[3]):
            inside = 0 <= y - (oy * s - p) < k and 0 <= x - (ox * s - p) < k
            if rp and inside:
                inside = (oy // rp) == (y // rp)           # a stacked map's taps stop at its own rows
            touched[n, :, oy, ox] = inside
    _same_outside(got, base, touched, "direct/%s/%s %s" % (name, where, form))
    assert torch.isfinite(got.cpu()[~touched]).all()
    if "w" not in dirs:
        return
    # one +inf in dy[n, co, y, x]: only row co of dw and db[co] may change
    data = R.direct_data(case, "gauss", seed=6)
    (dw0, db0), _ = direct_run(direct, case, place(data, cuda), "wgrad")
    co = Cout // 2
    oy, ox = (data["dy"].shape[2] // 2, data["dy"].shape[3] // 2) if where == "interior" else (0, 0)
    data["dy"][B - 1, co, oy, ox] = float("inf")
    (dw1, db1), form = direct_run(direct, case, place(data, cuda), "wgrad")
    rows = torch.zeros(dw0.shape, dtype=torch.bool); rows[co] = True
    _same_outside(dw1, dw0, rows, "direct/%s/wgrad %s" % (name, form))
    _same_outside(db1, db0, rows[:, 0, 0, 0], "direct/%s/db" % name)


@pytest.mark.parametrize("name", ["partial_block", "forced_split", "persistent", "stack3", "wgrad_splits2", "wgrad_two_images"])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_wino_planted_inf_stays_in_its_tiles(cuda, native_mod, name, where):
    case = _case(R.WINO_CASES, name)
    _, B, C, H, W, M, maps, env, dirs, expect = case
    if "f" in dirs:
        data = R.wino_data(case, "gauss", seed=5)
        base, _ = wino_run(native_mod, case, place(data, cuda), "fwd_leaky")
        ph = 7 if maps else H                            # a stacked map is a 7 x 7 image of its own (run as 8 x 8: row / column 7 are padding)
        y, x = (H // 2, W // 2) if where == "interior" else (H - 1, W - 1)
        data["x"][B - 1, C // 2, y, x] = float("inf")
        got, form = wino_run(native_mod, case, place(data, cuda), "fwd_leaky")
        # the tiles whose 4 x 4 patch (rows 2 ty - 1 .. 2 ty + 2 of the map) holds the pixel
        touched = torch.zeros(base.shape, dtype=torch.bool)
        my, y0 = (y // ph) * ph, y % ph
        for ty in range((ph + 1) // 2):
            for tx in range((W + 1) // 2):
                if 2 * ty - 1 <= y0 <= 2 * ty + 2 and 2 * tx - 1 <= x <= 2 * tx + 2:
                    touched[B - 1, :, my + 2 * ty:min(my + 2 * ty + 2, my + ph), 2 * tx:2 * tx + 2] = True
        g, b = got.cpu(), base.cpu()
        assert torch.equal(bits(g)[~touched], bits(b)[~touched]), "wino/%s %s: an output outside the pixel's tiles changed" % (name, form)
        assert not torch.isfinite(g[touched]).all()
    if "w" in dirs:
        data = R.wino_data(case, "gauss", seed=6)
        (dw0, db0), _ = wino_run(native_mod, case, place(data, cuda), "wgrad")
        co = M // 2
        oy, ox = (H // 2, W // 2) if where == "interior" else (0, 0)
        data["dy"][B - 1, co, oy, ox] = float("inf")
        (dw1, db1), form = wino_run(native_mod, case, place(data, cuda), "wgrad")
        rows = torch.zeros(dw0.shape, dtype=torch.bool); rows[co] = True
        _same_outside(dw1, dw0, rows, "wino/%s/wgrad %s" % (name, form))
        _same_outside(db1, db0, rows[:, 0, 0, 0], "wino/%s/db" % name)
