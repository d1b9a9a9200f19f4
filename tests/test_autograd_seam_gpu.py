"""Every torch.autograd.Function of scda_amd/autograd_ops.py and the modules of scda_amd/layers.py in the forms torch hands them tensors
in -- the table and the presentations of tests/seam_cases.py (checked on the CPU by tests/test_seam_cases.py) -- against float64:

* in every presentation (contiguous; strided views; contiguous views 4 bytes off a 16-byte boundary; strided, offset and stride-0
  grad_output; 0-dim upstream gradients from a product and from a plain tensor) the output and every gradient meet the tolerance rule of
  the kernel's family: tests/test_nn_ops_edges_gpu.py (check), rule A of tests/test_conv_edges_gpu.py (check_rule_a), tests/
  test_roi_edges_gpu.py (check, bit equality for RoI pooling, the per-pixel bound of the RoIAlign backward).  The helpers are imported;
* where the Function copies the operand (strided inputs, strided / stride-0 grad_output) the kernels see the same values at the same
  alignment: bit equality with the contiguous presentation.  An offset operand may select another kernel form: the float64 rule only,
  and the form where the code exposes it;
* gradient routing: every subset of required gradients gives the bits of the all-inputs run; parameters in a scda_amd.flat bucket
  receive pre-fill + gradient inside the slice, nothing outside it, and autograd receives None.
Each comparison prints an `EDGE` line (pytest -s); the worst figure per Function goes to profiles/autograd_seam.txt."""
import contextlib
import copy
import functools
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

import seam_cases as S
from test_conv_edges_gpu import FACTOR, _stop_after_a_device_fault, check_rule_a  # noqa: F401  (the fixture is autouse here too)
from test_nn_ops_edges_gpu import bits, check as nn_check
from test_roi_edges_gpu import check as roi_check, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in S.CASES]
WORST = {}              # Function / module -> (error / bound, error, bound, label)
_EDGE = re.compile(r"EDGE (.*) E32=\S+ kernel=(\S+) bound=(\S+)")


def note(owner, label, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    if owner not in WORST or ratio > WORST[owner][0]:
        WORST[owner] = (ratio, err, bound, label)


def ruled(owner, helper, *args, **kw):
    """run one of the imported tolerance helpers; its EDGE lines are printed as they are and their figures kept for the profile"""
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            helper(*args, **kw)
    finally:
        text = buf.getvalue()
        sys.stdout.write(text)
        for label, err, bound in _EDGE.findall(text):
            note(owner, label, float(err), float(bound))


@pytest.fixture(scope="module", autouse=True)
def _profile():
    """profiles/autograd_seam.txt: one line per Function / module this run compared, the file replaced by each run"""
    yield
    if WORST:
        with open(os.path.join(ROOT, "profiles", "autograd_seam.txt"), "w") as f:
            for owner in sorted(WORST):
                ratio, err, bound, label = WORST[owner]
                f.write("%s: worst error %.3e bound %.3e (%.2f of the bound) at %s\n" % (owner, err, bound, ratio, label))


@pytest.fixture
def mods(cuda):
    from scda_amd import autograd_ops as A, native as N
    return A, N


@contextlib.contextmanager
def env_of(case_env):
    with pytest.MonkeyPatch.context() as m:
        for k, v in case_env.items():
            m.setenv(k, v)
        yield


# ---------------------------------------------------------------- which kernel form ran
def _aligned(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


@contextlib.contextmanager
def proving(N, log):
    """Inside the block every convolution / GEMM launch the Functions make through scda_amd.native proves its form right behind the
    launch, as tests/test_conv_edges_gpu.py does: native.last_plan() against the decision launch_plan.h gives for the call
    (native.plan_conv / plan_gemm with the alignment of the operands that select the staging: an unaligned dy takes the register-staged
    weight gradient, unaligned GEMM operands the register-staged kernel), the Winograd launches native.wino_last_order() /
    wino_last_persistent() against native.plan_wino.  log collects one line per proved launch."""
    o = {k: getattr(N, k) for k in ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv2d_wgrad_bias", "gemm", "conv2d_wino",
                                    "conv2d_wino_pool", "conv2d_wino_wgrad")}

    def proved(direction, geom, al=True):
        plan, lp = N.plan_conv(direction, *geom, aligned=al), N.last_plan()
        assert lp[:3] == (plan["bm"], plan["bn"], plan["splits"]) and (lp[3] is True) == (plan["family"] == 1), (direction, geom, al, lp, plan)
        if not al:
            assert lp[3] is False, (direction, geom, lp)           # the register-staged kernel ran
        log.append("%s:fam%d,%dx%d,s%d%s" % (direction, plan["family"], plan["bm"], plan["bn"], plan["splits"], "" if al else ",unaligned"))

    def fwd(x, w, bias, stride, pad, act=0, slope=0.01, row_period=0):
        y = o["conv2d_fwd"](x, w, bias, stride, pad, act, slope, row_period=row_period)
        B, Cin, IH, IW = x.shape
        if not N.wino_ok(B, Cin, IH, IW, w.shape[0], w.shape[2], w.shape[3], stride, pad, row_period):
            proved("fwd", (B, Cin, IH, IW, w.shape[0], w.shape[2], stride, pad, row_period))
        return y

    def dgrad(dy, w, x_shape, stride, pad, act_src=None, act_slope=0.0, row_period=0):
        dx = o["conv2d_dgrad"](dy, w, x_shape, stride, pad, act_src=act_src, act_slope=act_slope, row_period=row_period)
        B, Cin, IH, IW = x_shape
        Cout, _, KH, KW = w.shape
        if N._route(1, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)[0]:
            return dx
        if act_src is None and Cin <= 4 and Cout * KH * KW * 16 <= 65536 and (KH, KW) in ((3, 3), (1, 1)):
            log.append("dgrad:small_cin")           # (conv_dgrad_small_cin_kernel: no tiles, no plan)
        else:
            proved("dgrad", (B, Cin, IH, IW, Cout, KH, stride, pad, row_period))
        return dx

    def wgrad(dy, x, w_shape, stride, pad, out=None, row_period=0):
        dw = o["conv2d_wgrad"](dy, x, w_shape, stride, pad, out=out, row_period=row_period)
        B, Cin, IH, IW = x.shape
        if not N.wino_wgrad_ok(B, Cin, IH, IW, w_shape[0], w_shape[2], w_shape[3], stride, pad, row_period):
            proved("wgrad", (B, Cin, IH, IW, w_shape[0], w_shape[2], stride, pad, row_period), _aligned(dy))
        return dw

    def wgrad_bias(dy, x, w_shape, stride, pad, out=None, db_out=None, row_period=0):
        r = o["conv2d_wgrad_bias"](dy, x, w_shape, stride, pad, out=out, db_out=db_out, row_period=row_period)
        B, Cin, IH, IW = x.shape
        fusable = bool(N.lib().scda_conv2d_wgrad_bias_fusable(B, w_shape[0], dy.shape[2], dy.shape[3], dy.data_ptr()))
        assert fusable <= ((dy.shape[2] * dy.shape[3]) % 16 == 0 and _aligned(dy))
        if fusable and not N.wino_wgrad_ok(B, Cin, IH, IW, w_shape[0], w_shape[2], w_shape[3], stride, pad, row_period):
            proved("wgrad_bias", (B, Cin, IH, IW, w_shape[0], w_shape[2], stride, pad, row_period))
        return r            # (not fusable: conv2d_wgrad above proved its launch, the bias gradient is a reduction without a plan)

    def gemm(a, b, M, N_, K, lda, ldb, trans_a=False, trans_b=False, *args, **kw):
        c = o["gemm"](a, b, M, N_, K, lda, ldb, trans_a, trans_b, *args, **kw)
        al = _aligned(a, b)
        plan, lp = N.plan_gemm(M, N_, K, lda, ldb, trans_a, trans_b, aligned=al), N.last_plan()
        fam = 2 if lp[3] == 2 else 1 if lp[3] else 0
        assert lp[:2] == (plan["bm"], plan["bn"]) and fam == plan["family"] and lp[2] == (-1 if plan["x9_stream"] else plan["splits"]), (lp, plan)
        if not al:
            assert fam == 0, (lp, plan)                                 # unaligned operands: the register-staged kernel
        log.append("gemm:fam%d,%dx%d,s%d%s" % (fam, lp[0], lp[1], lp[2], "" if al else ",unaligned"))
        return c

    def wino_proved(kind, B, cin, H, W, cout, rp):
        plan = N.plan_wino(kind, B, cin, H, W, cout, rp)
        order, persistent = N.wino_last_order()[0], N.wino_last_persistent()
        assert order == (plan["mb"], bool(plan["pixel_major"]), plan["gm"], plan["splits"]) and persistent == bool(plan["persist"]), (kind, order, persistent, plan)
        log.append("wino %s:mb%d,gm%d,s%d%s" % (kind, order[0], order[2], order[3], ",persistent" if persistent else ""))

    def wino(x, u, bias, M, act=0, slope=0.01, mask_src=None, mask_slope=0.0, for_dgrad=False, row_period=0):
        y = o["conv2d_wino"](x, u, bias, M, act, slope, mask_src, mask_slope, for_dgrad=for_dgrad, row_period=row_period)
        B, C, H, W = x.shape
        if for_dgrad:
            wino_proved("dgrad_mask" if mask_src is not None else "dgrad", B, M, H, W, C, row_period)
        else:
            wino_proved("fwd", B, C, H, W, M, row_period)
        return y

    def wino_pool(x, u, bias, M, act=0, slope=0.01):
        r = o["conv2d_wino_pool"](x, u, bias, M, act, slope)
        wino_proved("fwd_pool", x.shape[0], x.shape[1], x.shape[2], x.shape[3], M, 0)
        return r

    def wino_wgrad(dy, x, w_shape, out=None, db_out=None, want_bias=False, row_period=0):
        r = o["conv2d_wino_wgrad"](dy, x, w_shape, out=out, db_out=db_out, want_bias=want_bias, row_period=row_period)
        B, Cin, H, W = x.shape
        kind = "wgrad_bias" if (want_bias or db_out is not None) else "wgrad"
        plan, order = N.plan_wino(kind, B, Cin, H, W, w_shape[0], row_period), N.wino_last_order()[1]
        assert order == (plan["splits"], plan["order"]), (kind, order, plan)
        log.append("wino %s:s%d,o%d" % ((kind,) + order))
        return r

    with pytest.MonkeyPatch.context() as m:
        for k, f in (("conv2d_fwd", fwd), ("conv2d_dgrad", dgrad), ("conv2d_wgrad", wgrad), ("conv2d_wgrad_bias", wgrad_bias), ("gemm", gemm),
                     ("conv2d_wino", wino), ("conv2d_wino_pool", wino_pool), ("conv2d_wino_wgrad", wino_wgrad)):
            m.setattr(N, k, f)
        yield log


FORMS = []              # the proved launches of the most recent run of a conv-family case or module


# ---------------------------------------------------------------- running a case
def place(case, cuda, how, requires):
    """the case's inputs on the device, input k in the form how.get(k, "base"); `requires` as leaves that require grad"""
    T = {}
    for k, v in case.inputs.items():
        form = how.get(k, "base")
        t = S.base(v, cuda) if form == "base" else S.offset(v, cuda) if form == "offset" else S.STRIDED[case.strided.get(k, "cols")](v, cuda)
        T[k] = t.detach().requires_grad_() if k in requires else t
    return T


def upstream(case, y, form, cuda):
    """the grad_output of the run in the form asked for, and the same gradient as a host tensor for the references"""
    if case.loss:
        return None
    dy = case.dy(tuple(y.shape))
    if form == "strided":
        return S.every_other_column(dy, cuda)
    if form == "offset":
        return S.offset(dy, cuda)
    return dy.to(cuda)


def host_dy(case, out_shape, form):
    """what the device run's upstream gradient is worth, on the host"""
    if case.loss:
        return {"base": 1.0, "mul2": 2.0, "plain": 0.75}[form]
    return torch.ones(out_shape) if form in ("stride0", "ones") else case.dy(tuple(out_shape))


def run(case, A, cuda, how=None, dy_form="base", requires=None):
    """forward and backward of one case -> (y, {input: gradient}, T)"""
    requires = case.diff if requires is None else requires
    del FORMS[:]
    with env_of(case.env), (proving(A.N, FORMS) if case.family == "conv" else contextlib.nullcontext()):
        T = place(case, cuda, how or {}, requires)
        y = case.run(A, T)
        if case.loss:
            if dy_form == "mul2":
                (y * 2.0).backward()
            elif dy_form == "plain":
                y.backward(torch.tensor(0.75, device=cuda))
            else:
                y.backward()
        elif dy_form == "stride0":
            y.sum().backward()
        elif dy_form == "ones":
            y.backward(torch.ones(y.shape, device=cuda))
        else:
            y.backward(upstream(case, y, dy_form, cuda))
    return y.detach(), {k: T[k].grad for k in requires}, T


@functools.lru_cache(maxsize=None)
def keep_of(name):
    """the keep decisions of a dropout-bearing case: read back from DropoutSeededFn on ones"""
    from scda_amd import autograd_ops as A
    case = S.BY_NAME[name]
    p, seed = case.keep
    ones = torch.ones(case.inputs["x"].shape, device="cuda:0")
    return (A.DropoutSeededFn.apply(ones, p, seed, False) != 0).cpu()


@functools.lru_cache(maxsize=None)
def reference(name, dy_form, out_shape):
    """-> the references of a case under one upstream gradient, computed once and shared"""
    case = S.BY_NAME[name]
    dy = host_dy(case, out_shape, dy_form)
    if case.family == "conv":
        v64, mag = case.conv_ref(case, dy, torch.float64)
        v32, _ = case.conv_ref(case, dy, torch.float32)
        return v64, v32, mag
    if case.family == "roi":
        return case.roi_ref(case, dy)
    out = []
    for dt in (torch.float64, torch.float32):
        T = case.host(dt)
        if case.keep:
            T["keep"] = keep_of(name)
        y = case.ref(T)
        g = torch.autograd.grad(y, [T[k] for k in case.diff], (dy.to(dt) if torch.is_tensor(dy) else torch.tensor(dy, dtype=dt)))
        out.append({"y": y.detach(), **{k: v for k, v in zip(case.diff, g)}})
    return tuple(out)


def against_fp64(case, label, y, grads, dy_form):
    """the family's rule on the output and on every requested gradient"""
    ref = reference(case.name, dy_form, tuple(y.shape))
    got = {"y": y, **grads}
    for key, val in got.items():
        tag = "%s %s [%s]" % (case.name, key, label)
        if case.family == "conv":
            v64, v32, mag = ref
            fam = "wino" if case.fn == "ConvPoolFn" else "gemm" if case.fn == "LinearFn" else "direct"
            ruled(case.fn, check_rule_a, tag, fam, val, lambda dt, k=key: ((v64 if dt == torch.float64 else v32)[k], mag[k]), case.K[key], FACTOR[fam])
        elif case.fn == "RoIPoolFn":
            same(val.cpu().numpy(), ref["out" if key == "y" else "grad"], tag)
            note(case.fn, tag, 0.0, 0.0)
        elif case.family == "roi":
            if key == "y":
                ruled(case.fn, roi_check, tag, val.cpu().numpy(), ref["out64"], ref["out32"])
            else:           # the per-pixel bound of tests/test_roi_edges_gpu.py::test_roi_align_bwd_inexact
                err = np.abs(val.cpu().numpy() - ref["grad64"])
                bound = (ref["k"] + 2) * 2.0 ** -24 * ref["S"]
                worst = float((err / np.maximum(bound, 1e-300)).max())
                print("\nEDGE %s kmax=%d worst_err/bound=%.3e max_err=%.3e" % (tag, int(ref["k"].max()), worst, err.max()))
                note(case.fn, tag, float(err.max()), float(err.max() / worst) if worst > 0 else 0.0)
                assert (err <= bound).all(), (tag, worst)
        else:
            r64, r32 = ref
            v = val.reshape(1) if val.dim() == 0 else val
            ruled(case.fn, nn_check, tag, v, r64[key].reshape(v.shape), r32[key].reshape(v.shape))


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), "%s: not the bits of the contiguous presentation" % (what,)


def strided_names(case):
    """presentation b: every float input and the integer targets (inputs of one element have no strided form)"""
    return [k for k, v in case.inputs.items() if (v.dtype == torch.float32 or k == "targets") and v.numel() > 1 and k not in case.no_strided]


RUN_CASES = [c for c in S.CASES if not c.forward_only]
RUN_IDS = [c.name for c in RUN_CASES]


# ---------------------------------------------------------------- a - d: the presentations
@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_input_presentations(cuda, mods, case, monkeypatch):
    A, N = mods
    cls = getattr(A, case.fn)
    counted = []
    inner = cls.backward
    monkeypatch.setattr(cls, "backward", staticmethod(lambda ctx, *g: counted.append(inner(ctx, *g)) or counted[-1]))
    y0, g0, T0 = run(case, A, cuda)
    n_args = S.forward_arity(cls) or 2 + 3 * 2          # (AdvLossFn: scale, k and three tensors for each of its two groups here)
    assert counted and all(isinstance(r, tuple) and len(r) == n_args or n_args == 1 and torch.is_tensor(r) for r in counted), \
        "%s.backward returned %s values for %d forward arguments" % (case.fn, [len(r) if isinstance(r, tuple) else 1 for r in counted], n_args)
    against_fp64(case, "base", y0, g0, "base")
    for k in case.diff:             # the layout of a returned gradient
        assert g0[k].shape == T0[k].shape
    # b: one strided operand at a time
    for k in strided_names(case):
        if k in case.refuses_strided:
            with pytest.raises(case.refuses_strided[k] or ValueError):
                run(case, A, cuda, {k: "strided"})
            torch.cuda.synchronize()
            continue
        y, g, T = run(case, A, cuda, {k: "strided"})
        assert not T[k].is_contiguous()
        against_fp64(case, "strided " + k, y, g, "base")
        same_bits(y, y0, "%s output, strided %s" % (case.name, k))
        for d in case.diff:
            same_bits(g[d], g0[d], "%s gradient of %s, strided %s" % (case.name, d, k))
            if d == k and d in case.keeps_strides:      # what backward() itself returned, before autograd lays it out
                ret = counted[-1][list(case.inputs).index(d)]
                assert ret.stride() == T[d].stride() and g[d].stride() == T[d].stride(), (case.name, d, ret.stride(), T[d].stride())
    # c: one operand at a time 4 bytes off a 16-byte boundary, then all of them
    floats = case.float_inputs()
    for which in [(k,) for k in floats] + ([tuple(floats)] if len(floats) > 1 else []):
        label = "offset " + ("+".join(which) if len(which) == 1 else "all")
        if set(which) & set(case.refuses_offset):       # float4-only launches: the launcher refuses, nothing runs
            with pytest.raises(N.ScdaNativeError, match="align"):
                run(case, A, cuda, {k: "offset" for k in which})
            torch.cuda.synchronize()
            continue
        y, g, T = run(case, A, cuda, {k: "offset" for k in which})
        assert all(T[k].data_ptr() % 16 == 4 and T[k].is_contiguous() for k in which)
        if case.family == "conv":       # every launch proved its form against launch_plan.h's decision for these operands (proving)
            print("\nEDGE %s [%s] forms: %s" % (case.name, label, " ".join(FORMS)))
            assert len(FORMS) >= 3, FORMS
            if case.fn == "LinearFn" and set(which) & {"x", "w"}:
                assert any(f.endswith(",unaligned") for f in FORMS), FORMS
        against_fp64(case, label, y, g, "base")


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_grad_output_presentations(cuda, mods, case, monkeypatch):
    A, N = mods
    y0, g0, _ = run(case, A, cuda)
    if case.loss:
        for form in ("mul2", "plain"):
            y, g, _ = run(case, A, cuda, dy_form=form)
            same_bits(y, y0, case.name + " loss")
            against_fp64(case, "g " + form, y, g, form)
        return
    seen = []
    cls = getattr(A, case.fn)
    inner = cls.backward
    monkeypatch.setattr(cls, "backward", staticmethod(lambda ctx, *g: seen.append((g[0].is_contiguous(), g[0].stride(), g[0].data_ptr() % 16)) or inner(ctx, *g)))
    y, g, _ = run(case, A, cuda, dy_form="strided")
    assert seen[-1][0] is False                                       # backward() did receive the strided gradient
    against_fp64(case, "dy strided", y, g, "base")
    for d in case.diff:
        same_bits(g[d], g0[d], "%s gradient of %s, strided dy" % (case.name, d))
    y, g, _ = run(case, A, cuda, dy_form="offset")
    assert seen[-1][0] is True and seen[-1][2] == 4
    if case.family == "conv":
        print("\nEDGE %s [dy offset] forms: %s" % (case.name, " ".join(FORMS)))
        assert len(FORMS) >= 3, FORMS
        if case.fn != "ConvPoolFn" and case.env.get("SCDA_WINOGRAD") == "0":        # an activation's act_bwd hands on a fresh dy
            assert ("leaky" in case.name) != any(f.startswith("wgrad") and f.endswith(",unaligned") for f in FORMS), FORMS
    against_fp64(case, "dy offset", y, g, "base")
    if case.forms == "norm_up":         # an offset dy takes upsample2x_bwd + the norm's backward, an aligned one the fused launch:
        for d in case.diff:             # the docstrings promise the same bits from either
            same_bits(g[d], g0[d], "%s gradient of %s, two-launch backward" % (case.name, d))
        assert not N.aligned16(S.offset(case.dy(tuple(y.shape)), cuda)) and N.aligned16(upstream(case, y, "base", cuda))
        monkeypatch.setenv("SCDA_NO_NORM_UP_BWD_FUSION", "1")
        _, g2, _ = run(case, A, cuda)
        monkeypatch.delenv("SCDA_NO_NORM_UP_BWD_FUSION")
        for d in case.diff:
            same_bits(g2[d], g0[d], "%s gradient of %s, fusion switched off" % (case.name, d))
    if case.forms == "bn_join":         # an offset dy is cloned to an aligned one: the same launch on the same values
        for d in case.diff:
            same_bits(g[d], g0[d], "%s gradient of %s, offset dy" % (case.name, d))
    y1, g1, _ = run(case, A, cuda, dy_form="ones")
    y, g, _ = run(case, A, cuda, dy_form="stride0")
    assert set(seen[-1][1]) == {0}                                    # ... and the stride-0 one
    against_fp64(case, "dy stride 0", y, g, "stride0")
    for d in case.diff:
        same_bits(g[d], g1[d], "%s gradient of %s, stride-0 dy" % (case.name, d))


CHAINED = [c for c in S.CASES if c.chain is not None]


@pytest.mark.parametrize("case", CHAINED, ids=[c.name for c in CHAINED])
def test_fused_functions_give_the_bits_of_their_chain(cuda, mods, case):
    """the dropout-bearing and fused Functions against the chain of Functions their docstrings name, bit for bit in both directions"""
    A, N = mods
    y0, g0, _ = run(case, A, cuda)
    chained = copy.copy(case)
    chained.run = case.chain
    y, g, _ = run(chained, A, cuda)
    same_bits(y, y0, case.name + " output against its chain")
    for d in case.diff:
        same_bits(g[d], g0[d], "%s gradient of %s against its chain" % (case.name, d))


def test_maxpool3x3s2_is_forward_only(cuda, mods):
    A, N = mods
    case = S.BY_NAME["maxpool3x3s2[2x3x7x9]"]
    want = case.ref(case.host(torch.float32, requires=()))
    for how in ({}, {"x": "strided"}, {"x": "offset"}):
        T = place(case, cuda, how, ())
        assert torch.equal(bits(case.run(A, T)), bits(want)), how
    note(case.fn, case.name + " y (bit for bit)", 0.0, 0.0)
    T = place(case, cuda, {}, ("x",))
    with pytest.raises(NotImplementedError, match="no backward"):
        case.run(A, T).sum().backward()
    assert T["x"].grad is None


# ---------------------------------------------------------------- e: which gradients are asked for
MULTI = [c for c in RUN_CASES if len(c.diff) > 1]


@pytest.mark.parametrize("case", MULTI, ids=[c.name for c in MULTI])
def test_every_subset_of_required_gradients(cuda, mods, case):
    A, N = mods
    y0, g0, _ = run(case, A, cuda)
    differ = []
    for subset in case.subsets()[:-1]:
        y, g, T = run(case, A, cuda, requires=subset)
        same_bits(y, y0, "%s output, gradients of %s" % (case.name, subset))
        for d in case.diff:
            if d not in subset:
                assert T[d].grad is None and not T[d].requires_grad
            elif not torch.equal(bits(g[d]), bits(g0[d])):
                rel = ((g[d] - g0[d]).abs().max() / g0[d].abs().max()).item()
                print("\nEDGE %s gradient of %s with only %s required: differs from the all-inputs run by %.3e of its largest value"
                      % (case.name, d, "+".join(subset), rel))
                differ.append((d, subset, rel))
    assert not differ, "%s: gradients that depend on which others were asked for: %s" % (case.name, differ)


# ---------------------------------------------------------------- f: parameters in a flat bucket
GUARD_WORD = 0x7FC5A5A5
BUCKETED = [c for c in RUN_CASES if c.bucket]


class Holder(torch.nn.Module):
    """guard words, the bucketed parameters, guard words"""
    def __init__(self, params, cuda):
        super().__init__()
        self.g0 = torch.nn.Parameter(torch.zeros(8, device=cuda))
        for k, v in params.items():
            setattr(self, k, torch.nn.Parameter(v.to(cuda)))
        self.g1 = torch.nn.Parameter(torch.zeros(8, device=cuda))


def bucket_variants(case):
    """(parameters in the bucket, inputs that require grad, lazily-zeroed slices)"""
    out = [(case.bucket, case.diff, ())]
    if case.family == "conv":           # Conv2dFn / ConvPoolFn: weight + bias, weight only, bias only; LinearFn: and the overwrite
        out += [(case.bucket, ("w",), ()), (case.bucket, ("b",), ()), (case.bucket, ("x", "w"), ())]
        if case.fn == "LinearFn":
            out.append((case.bucket, case.diff, ("w",)))
    else:                               # the batch norms: one of gamma / beta in a bucket (`both` is false)
        out += [(("gamma",), case.diff, ()), (("beta",), case.diff, ())]
    return [(b, r, f) for b, r, f in out if set(r) <= set(case.diff)]


@pytest.mark.parametrize("case", BUCKETED, ids=[c.name for c in BUCKETED])
def test_parameters_in_a_flat_bucket(cuda, mods, case):
    from scda_amd.flat import FlatParams
    A, N = mods
    for in_bucket, requires, fresh in bucket_variants(case):
        tag = "%s bucket=%s requires=%s%s" % (case.name, "+".join(in_bucket), "+".join(requires), " fresh=" + "+".join(fresh) if fresh else "")
        y0, plain, _ = run(case, A, cuda, requires=requires)
        holder = Holder({k: case.inputs[k] for k in in_bucket}, cuda)
        flat = FlatParams(holder)
        pre = torch.randn(flat.numel, generator=S.gen(7))
        flat.grad.copy_(pre)
        flat.grad.view(torch.int32)[:8] = GUARD_WORD
        flat.grad.view(torch.int32)[-8:] = GUARD_WORD
        before = bits(flat.grad).clone()
        handed = []
        with env_of(case.env):
            T = place(case, cuda, {}, [k for k in requires if k not in in_bucket])
            for k in in_bucket:
                p = getattr(holder, k)
                assert p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0 and p._scda_flat is flat
                p.requires_grad_(k in requires)
                if k in requires:
                    p.register_hook(lambda g, k=k: handed.append(k) if g is not None else None)
                if k in fresh:
                    flat.fresh.add(id(p))
                T[k] = p
            y = case.run(A, T)
            y.backward(upstream(case, y, "base", cuda))
        torch.cuda.synchronize()
        # (a batch norm with only one of gamma / beta in the bucket allocates both gradients and hands them to autograd, which adds
        # the bucketed one into its slice: the slice still ends as pre-fill + gradient)
        through_autograd = [k for k in in_bucket if k in requires] if case.family == "nn" and len(in_bucket) < len(case.bucket) else []
        assert sorted(handed) == sorted(through_autograd), "%s: autograd was handed a gradient for %s" % (tag, handed)
        same_bits(y.detach(), y0, tag + " output")
        after = bits(flat.grad)
        touched = torch.zeros(flat.numel, dtype=torch.bool)
        for k in in_bucket:
            p = getattr(holder, k)
            lo = flat.offset[id(p)]
            sl = slice(lo, lo + p.numel())
            if k not in requires:
                continue
            touched[sl] = True
            got = flat.grad[sl].cpu().double()
            if k in fresh:
                assert torch.equal(bits(flat.grad[sl]), bits(plain[k].reshape(-1))), tag + ": an overwritten slice is the plain gradient"
                continue
            want = pre[sl].double() + plain[k].reshape(-1).cpu().double()
            err = (got - want).abs()
            bound = 2.0 ** -24 * want.abs()             # one fp32 rounding of pre-fill + gradient
            worst = float((err / bound.clamp_min(1e-300)).max())
            print("\nEDGE %s slice of %s: worst error / rounding of the sum = %.3f (max error %.3e)" % (tag, k, worst, err.max().item()))
            assert (err <= bound).all(), "%s: slice of %s is not pre-fill + gradient within one rounding (%.3f roundings)" % (tag, k, worst)
        assert torch.equal(after[~touched], before[~touched]), tag + ": a word outside the slices of the required parameters changed"
        assert (after[:8] == GUARD_WORD).all() and (after[-8:] == GUARD_WORD).all()
        for k in requires:
            if k not in in_bucket:
                same_bits(T[k].grad, plain[k], "%s gradient of %s" % (tag, k))


# ---------------------------------------------------------------- the modules
def _module_ref(name, m, host, dy, dtype, family):
    T = {k: v.clone().to(dtype) for k, v in host.items()}
    leaves = [k for k in ("x", "residual", "weight", "bias") if k in T and (k in ("x", "residual") or getattr(m, k, None) is not None)]
    if "forward_add_relu" not in name:
        leaves = [k for k in leaves if k != "residual"]
    if name.startswith("BatchNorm2d") and not m.training:
        leaves = [k for k in leaves if k not in ("weight", "bias")]
    for k in leaves:
        T[k].requires_grad_()
    if family == "nn":
        y = S.module_reference(name, m, T)
        g = torch.autograd.grad(y, [T[k] for k in leaves], dy.to(dtype))
        return {"y": y.detach(), **dict(zip(leaves, g))}, None
    pre, act, slope = S.module_reference(name, m, T)
    y = S.act_t(pre, act, slope)
    g = torch.autograd.grad(y, [T[k] for k in leaves], dy.to(dtype), retain_graph=True)
    gpre = torch.autograd.grad(y, pre, dy.to(dtype))[0].abs()
    Tabs = {k: (v.detach().abs().requires_grad_() if k in leaves else v) for k, v in T.items()}
    Spre = S.module_reference(name, m, Tabs)[0]
    Sg = torch.autograd.grad(Spre, [Tabs[k] for k in leaves], gpre)
    return {"y": y.detach(), **dict(zip(leaves, g))}, {"y": Spre.detach(), **dict(zip(leaves, Sg))}


def _module_K(name, shape, m):
    if name.startswith("Linear"):
        return {"y": shape[1] + 1, "x": m.out_features, "weight": shape[0] + 1, "bias": shape[0] + 1}
    B, Cin, H, W = shape
    k = m.kernel_size[0]
    pixels = B * H * W
    if name.startswith("ConvTranspose"):
        return {"y": Cin + 1, "x": m.out_channels * k * k, "weight": pixels + 1, "bias": pixels * k * k + 1}
    return {"y": Cin * k * k + 1, "x": m.out_channels * k * k, "weight": pixels + 1, "bias": pixels + 1}


@pytest.mark.parametrize("entry", S.MODULES, ids=[e[0] for e in S.MODULES])
def test_modules_in_three_presentations(cuda, entry):
    from scda_amd import layers as L
    name, make, shape, family, env = entry
    torch.manual_seed(3)
    proto = make(L)
    host = {k: v.detach().clone() for k, v in proto.state_dict().items() if v.is_floating_point()}
    for k in ("weight", "bias", "running_mean", "running_var"):       # away from the initial ones and zeros
        if k in host:
            host[k] = torch.rand(host[k].shape, generator=S.gen(11 + len(k))) + 0.5 if k in ("weight", "running_var") and host[k].dim() == 1 \
                else host[k] + 0.1 * S.randn(host[k].shape, 17 + len(k))
    host["x"] = S.randn(shape, 21, 1.5, 0.2)
    join = "forward_add_relu" in name
    if join:
        host["residual"] = S.randn(shape, 22)
    base = {}
    for form in ("base", "strided", "offset"):
        m = copy.deepcopy(proto)
        m.load_state_dict({k: v for k, v in host.items() if k not in ("x", "residual")}, strict=False)
        m = m.to(cuda)
        put = {"base": S.base, "strided": S.transposed if len(shape) == 4 else S.every_other_column, "offset": S.offset}[form]
        x = put(host["x"], cuda).detach().requires_grad_()
        res = put(host["residual"], cuda).detach().requires_grad_() if join else None
        del FORMS[:]
        from scda_amd import native as N
        with env_of(env), (proving(N, FORMS) if family == "conv" else contextlib.nullcontext()):
            y = m.forward_add_relu(x, res) if join else m(x)
            dy = S.randn(tuple(y.shape), 23)
            y.backward(dy.to(cuda))
        if family == "conv":
            print("\nEDGE %s [%s x] forms: %s" % (name, form, " ".join(FORMS)))
            assert len(FORMS) >= 3, FORMS
            if name.startswith("Linear"):
                assert any(f.endswith(",unaligned") for f in FORMS) == (form == "offset"), FORMS
        got = {"y": y.detach(), "x": x.grad}
        if join:
            got["residual"] = res.grad
        got.update({k: p.grad for k, p in m.named_parameters() if p.grad is not None})
        assert form == "base" or (not x.is_contiguous() if form == "strided" else x.data_ptr() % 16 == 4)
        r64, mag = _module_ref(name, proto, host, dy, torch.float64, family)
        r32, _ = _module_ref(name, proto, host, dy, torch.float32, family)
        assert set(got) == set(r64), (name, sorted(got), sorted(r64))
        for key, val in got.items():
            tag = "%s %s [%s x]" % (name, key, form)
            if family == "conv":
                fam = "gemm" if name.startswith("Linear") else "direct"
                ruled("layers." + name, check_rule_a, tag, fam, val, lambda dt, k=key: ((r64 if dt == torch.float64 else r32)[k], mag[k]),
                      _module_K(name, shape, proto)[key], FACTOR[fam])
            else:
                ruled("layers." + name, nn_check, tag, val, r64[key], r32[key])
        if form == "base":
            base = got
        elif form == "strided" and name != "BatchNorm2d.forward_add_relu[train]":      # (that one documents another kernel for such a map)
            for key, val in got.items():
                same_bits(val, base[key], "%s %s, strided x" % (name, key))


# ---------------------------------------------------------------- the wrappers refuse before they launch
def test_loss_wrappers_refuse_wrong_shapes_before_the_launch(cuda, mods):
    """guards of scda_amd/native.py that run in front of the launch: the exception, a clean device, outputs untouched.  Every buffer
    handed over is as long as a launch would have read"""
    A, N = mods
    f = lambda *s: torch.randn(*s, device=cuda)
    R_, C_ = 9, 5
    logits, targets = f(R_, C_), torch.zeros(R_, dtype=torch.int64, device=cuda)
    long_t = torch.zeros(2 * R_, dtype=torch.int64, device=cuda)
    out2, probs = N.softmax_ce_fwd(logits, targets, -1)
    g = torch.ones(1, device=cuda)
    sentinel = torch.full((1,), 7.5, device=cuda)
    cases = [
        (ValueError, lambda: N.softmax_ce_fwd(logits, long_t, -1)),
        (ValueError, lambda: N.softmax_ce_bwd(probs, long_t, out2, g, -1)),
        (ValueError, lambda: N.softmax_ce_bwd(probs, long_t[::2], out2, g, -1)),                  # strided: the column of a label table
        (TypeError, lambda: N.softmax_ce_bwd(probs, long_t.int(), out2, g, -1)),
        (ValueError, lambda: N.smooth_l1_fwd(f(6, 8), f(8, 6), f(6, 8), 3.0, 1.0)),
        (ValueError, lambda: N.smooth_l1_fwd(f(6, 8), None, f(12, 8), 3.0, 1.0)),
        (ValueError, lambda: N.smooth_l1_bwd(f(6, 8), f(6, 8), f(8, 6), 3.0, 1.0, g)),
        (ValueError, lambda: N.smooth_l1_bwd(f(6, 8), f(6, 16)[:, ::2], f(6, 8), 3.0, 1.0, g)),
        (TypeError, lambda: N.smooth_l1_bwd(f(6, 8), None, f(6, 8).double(), 3.0, 1.0, g)),
        (ValueError, lambda: N.sigmoid_bce_rows_bwd(f(5, 33), f(7, 33), None, 1.0, g)),            # labels [1, n] or [C, n]
        (ValueError, lambda: N.sigmoid_bce_rows_bwd(f(5, 33), f(5, 66)[:, ::2], None, 1.0, g)),
        (ValueError, lambda: N.sigmoid_bce_rows_bwd(f(5, 33), f(1, 33), f(10), 1.0, g)),
        (TypeError, lambda: N.sigmoid_bce_rows_bwd(f(5, 33), f(1, 33).double(), None, 1.0, g)),
        (ValueError, lambda: N.sigmoid_bce_rows_fwd(f(5, 33), f(7, 33), None, 1.0, out=sentinel)),
        (ValueError, lambda: N.sigmoid_bce_rows_fwd(f(5, 33), f(1, 33), f(10), 1.0, out=sentinel)),
        (ValueError, lambda: N.bce_bwd(f(3, 85), f(3, 170), g)),
        (ValueError, lambda: N.linear_fwd(f(3, 20), f(7, 40), None)),
        (ValueError, lambda: N.linear_fwd(f(3, 20), f(7, 20), f(14))),
        (ValueError, lambda: N.linear_dgrad(f(3, 7), f(14, 20))),
        (ValueError, lambda: N.linear_wgrad(f(3, 7), f(6, 20))),
    ]
    for exc, call in cases:
        with pytest.raises(exc):
            call()
        torch.cuda.synchronize()
    assert sentinel.item() == 7.5
    dw = torch.full((2 * 7 * 20,), 7.5, device=cuda)
    with pytest.raises(ValueError):
        N.linear_wgrad(f(3, 7), f(3, 20), out=dw)
    torch.cuda.synchronize()
    assert (dw == 7.5).all()


def test_layer_wrappers_refuse_wrong_shapes_before_the_launch(cuda, mods):
    """the same for the layer wrappers the Functions reach: per-channel vectors of another length than the map's channels, operands of
    another size than the tensor that sizes the launch.  Every buffer is at least as long as the launch would have read or written"""
    A, N = mods
    from scda_amd import layers as L
    f = lambda *s: torch.randn(*s, device=cuda)
    x, dy = f(2, 4, 5, 5), f(2, 4, 5, 5)
    c4, c8 = (lambda: f(4).abs() + 0.5), (lambda: f(8).abs() + 0.5)
    rm, rv = torch.full((8,), 7.5, device=cuda), torch.full((8,), 7.5, device=cuda)
    x1 = f(1, 8, 7, 8)
    cases = [
        (ValueError, lambda: N.batchnorm_fwd(x, c8(), c4(), None, None, 1e-5, 0.1, 0, 0.0)),
        (ValueError, lambda: N.batchnorm_fwd(x, c4(), c4(), rm, rv, 1e-5, 0.1, 0, 0.0)),
        (ValueError, lambda: N.batchnorm_fwd(x, c4(), c4(), rm[::2], rv[::2], 1e-5, 0.1, 0, 0.0)),      # strided running statistics
        (TypeError, lambda: N.batchnorm_fwd(x, c4(), c4(), rm[:4].double(), rv[:4].double(), 1e-5, 0.1, 0, 0.0)),
        (ValueError, lambda: N.batchnorm_bwd(dy, x, c4(), c4(), c8(), c4(), 0, 0.0)),
        (ValueError, lambda: N.batchnorm_bwd(dy, x, c4(), c4(), c4(), c4(), 0, 0.0, out=(rm, rv))),
        (ValueError, lambda: N.batchnorm_bwd(f(2, 4, 5, 10), x, c4(), c4(), c4(), c4(), 0, 0.0)),
        (ValueError, lambda: N.batchnorm_add_relu_fwd(x1, f(1, 8, 7, 8), c8(), f(16), rm, rv, 1e-5, 0.1)),
        (ValueError, lambda: N.batchnorm_add_relu_fwd(x1, f(1, 8, 7, 8), c8(), c8(), f(16), f(16), 1e-5, 0.1)),
        (ValueError, lambda: N.batchnorm_add_relu_bwd(f(1, 8, 7, 8), x1, f(1, 8, 7, 8), c8(), c8(), f(16), c8())),
        (ValueError, lambda: N.batchnorm_add_relu_bwd(f(1, 8, 7, 8), x1, f(1, 8, 7, 16), c8(), c8(), c8(), c8())),
        (ValueError, lambda: N.batchnorm_eval(x, c4(), c4(), c8(), c8(), 1e-5, 0, 0.0)),
        (ValueError, lambda: N.batchnorm_eval(x, c4(), c4(), c4(), c4(), 1e-5, 0, 0.0, dy=f(2, 4, 5, 10))),
        (ValueError, lambda: N.instnorm_bwd(f(2, 4, 5, 10), x, f(8), f(8), 0, 0.0)),
        (ValueError, lambda: N.instnorm_bwd(dy, x, f(16), f(8), 0, 0.0)),
        (ValueError, lambda: N.axpby(f(3, 85), f(6, 85), 1.0, 1.0)),
        (ValueError, lambda: A.AddFn.apply(f(3, 85), f(6, 85))),
        (ValueError, lambda: N.dropout_apply(f(3, 85), torch.ones(6, 85, dtype=torch.uint8, device=cuda), 2.0)),
        (ValueError, lambda: N.dropout_seeded(f(3, 85), 0.5, 7, 2.0, relu_src=f(6, 85))),
        (ValueError, lambda: N.act_bwd(f(3, 85), f(6, 85), 0, 0.0)),
        (ValueError, lambda: N.maxpool2x2_bwd(f(2, 3, 6, 4), torch.zeros(2, 3, 6, 4, dtype=torch.uint8, device=cuda), (2, 3, 6, 8))),
        (ValueError, lambda: N.maxpool2x2_bwd(f(2, 3, 3, 4), torch.zeros(2, 3, 3, 4, dtype=torch.uint8, device=cuda), (2, 3, 6, 8), relu_y=f(2, 3, 6, 4))),
        (ValueError, lambda: N.conv2d_wino_pool(f(1, 32, 8, 8), f(1 << 16), f(128)[::2], 64)),
        (ValueError, lambda: N.conv2d_wino_pool(f(1, 32, 8, 8), f(1 << 16), f(128), 64)),
    ]
    for i, (exc, call) in enumerate(cases):
        with pytest.raises(exc):
            call()
        torch.cuda.synchronize()
    assert (rm == 7.5).all() and (rv == 7.5).all()
    bn = L.BatchNorm2d(4).to(cuda).train()          # the module: an 8-channel map would write 8 running statistics into 4
    with pytest.raises(ValueError, match="expected a"):
        bn(f(2, 8, 5, 5))
    torch.cuda.synchronize()
    assert not bn.running_mean.any() and (bn.running_var == 1).all()
