"""tests/seam_cases.py on the CPU: the table names every Function of scda_amd/autograd_ops.py, the presentations are what they claim, the
float64 references that are restatements agree with numerical differentiation, and every backward() returns one value per argument of
its forward().  The table itself runs on the device in tests/test_autograd_seam_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import seam_cases as S

CPU = torch.device("cpu")


def test_every_function_has_a_table_entry():
    from scda_amd import autograd_ops as A
    fns = S.functions_of(A)
    assert len(fns) >= 27 and "Conv2dFn" in fns
    named = {c.fn for c in S.CASES}
    assert not set(fns) - named, "autograd_ops Functions without an entry in tests/seam_cases.py: %s" % sorted(set(fns) - named)
    assert not named - set(fns), "entries for Functions that do not exist: %s" % sorted(named - set(fns))
    for c in S.CASES:
        assert set(c.diff) <= set(c.inputs) and set(c.bucket) <= set(c.diff), c.name
        assert all(v.numel() <= 300000 for v in c.inputs.values()), c.name      # a few hundred thousand elements at the most
    only_fwd = [c for c in S.CASES if c.forward_only]
    assert [c.fn for c in only_fwd] == ["MaxPool3x3s2Fn"]
    with pytest.raises(NotImplementedError):
        A.MaxPool3x3s2Fn.backward(None, torch.zeros(1))


def test_presentations_are_what_they_claim():
    for c in S.CASES:
        for k, t in c.inputs.items():
            assert S.base(t, CPU).is_contiguous() and S.base(t, CPU).data_ptr() % 16 == 0
            if t.dtype == torch.float32:            # (the offset form is the float operands': one element = 4 bytes)
                o = S.offset(t, CPU)
                assert torch.equal(o, t) and o.is_contiguous() and o.data_ptr() % 16 == 4, (c.name, k)
            if t.numel() < 2:
                continue
            v = S.STRIDED[c.strided.get(k, "cols")](t, CPU)
            assert torch.equal(v, t) and not v.is_contiguous() and v.shape == t.shape, (c.name, k)
        if c.strided.get("heat") == "t01":          # the keypoint head's view: R and Kp strided, every plane contiguous
            v = S.transposed01(c.inputs["heat"], CPU)
            assert v.stride()[2:] == (v.shape[3], 1) and v.stride(0) < v.stride(1)
    t = S.randn((2, 3, 5, 7), 1)
    v = S.transposed(t, CPU)
    assert torch.equal(v, t) and not v.is_contiguous() and v.stride() == (105, 35, 1, 5)
    g = S.stride0(0.75, (2, 3), CPU)
    assert g.stride() == (0, 0) and g.shape == (2, 3) and (g == 0.75).all()
    y = torch.zeros(2, 3, requires_grad=True)
    seen = []
    y.register_hook(lambda gr: seen.append(gr.stride()))
    y.sum().backward()
    assert seen == [(0, 0)]                          # what the stride-0 presentation stands for


def _keep_for(c):
    return torch.rand(c.inputs["x"].shape, generator=S.gen(5)) < 0.5


RESTATED = [c for c in S.CASES if c.restated and c.family == "nn"]


@pytest.mark.parametrize("case", RESTATED, ids=[c.name for c in RESTATED])
def test_restated_references_agree_with_numerical_differentiation(case):
    """the float64 references that are not one torch operator: their autograd gradient against torch.autograd.gradcheck"""
    T = case.host(torch.float64)
    if case.keep:
        T["keep"] = _keep_for(case)
    names = list(case.diff)

    def f(*leaves):
        return case.ref({**T, **dict(zip(names, leaves))})

    assert torch.autograd.gradcheck(f, tuple(T[k] for k in names), eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


def test_conv_pool_restatement_against_torch_autograd():
    """the Winograd restatement with the pool's scatter written out (seam_cases.conv_pool_ref) against torch's own chain in float64, on a
    small layer of the same structure"""
    c = S.Case("small", "ConvPoolFn", "conv", {"x": S.randn((1, 8, 4, 6), 1), "w": S.randn((5, 8, 3, 3), 2, 0.1), "b": S.randn((5,), 3)},
               ("x", "w", "b"), run=None)
    dy = S.randn((1, 5, 2, 3), 4)
    vals, mag = S.conv_pool_ref(c, dy, torch.float64)
    T = c.host(torch.float64)
    y = F.max_pool2d(F.relu(F.conv2d(T["x"], T["w"], T["b"], 1, 1)), 2, 2)
    g = torch.autograd.grad(y, [T["x"], T["w"], T["b"]], dy.double())
    for got, want, key in zip((vals["y"], vals["x"], vals["w"], vals["b"]), (y,) + g, "yxwb"):
        assert torch.allclose(got, want.detach(), rtol=1e-12, atol=1e-13), key
        assert (mag[key] + 1e-12 >= got.abs()).all(), key              # a magnitude sum bounds its element


def test_bilinear_magnitude_sums():
    """S of seam_cases.bilinear_ref is the magnitude sum tests/conv_refs.py states for the same layer"""
    import conv_refs as CR
    c = S.BY_NAME["conv[2x3x6x5->4,k1]"]
    dy = S.randn((2, 4, 6, 5), 7)
    vals, mag = c.conv_ref(c, dy, torch.float64)
    x, w, b = (c.inputs[k] for k in "xwb")
    y, Sy = CR.conv_fwd(x, w, b, 1, 0)
    dx, Sdx = CR.conv_dgrad(dy, w, x.shape, 1, 0)
    (dw, db), (Sw, Sb) = CR.conv_wgrad(dy, x, w.shape, 1, 0)
    for key, v, s in (("y", y, Sy), ("x", dx, Sdx), ("w", dw, Sw), ("b", db, Sb)):
        assert torch.allclose(vals[key], v, rtol=1e-12, atol=1e-13) and torch.allclose(mag[key], s, rtol=1e-12, atol=1e-13), key


def test_backward_returns_one_value_per_forward_argument():
    """read from the sources: every `return` of backward() lists as many values as forward() takes arguments.  AdvLossFn builds its
    tuple from the call's group count and MaxPool3x3s2Fn.backward only raises: tests/test_autograd_seam_gpu.py counts the first there"""
    from scda_amd import autograd_ops as A
    dynamic = []
    for name, cls in S.functions_of(A).items():
        n_fwd, n_bwd = S.forward_arity(cls), S.static_backward_arity(cls)
        if n_fwd is None or n_bwd is None:
            dynamic.append(name)
            continue
        assert n_fwd == n_bwd, "%s: forward takes %d arguments, backward returns %d values" % (name, n_fwd, n_bwd)
    assert sorted(dynamic) == ["AdvLossFn", "MaxPool3x3s2Fn"], dynamic


def test_module_table_builds_on_the_cpu():
    from scda_amd import layers as L
    for name, make, shape, family, env in S.MODULES:
        m = make(L)
        T = {k: v.detach().double() for k, v in m.state_dict().items() if v.is_floating_point()}
        T["x"] = S.randn(shape, 3).double()
        T["residual"] = S.randn(shape, 4).double()
        out = S.module_reference(name, m, T)
        out = out[0] if isinstance(out, tuple) else out
        assert torch.isfinite(out).all() and out.shape[0] == shape[0], name
