"""The seam between torch and the kernels: one table with an entry for every torch.autograd.Function of scda_amd/autograd_ops.py, the forms
("presentations") in which torch can hand a tensor to one, and the float64 reference of each entry.  No device is needed to import this
file; tests/test_seam_cases.py checks it on the CPU, tests/test_autograd_seam_gpu.py runs the table on the device.

A Case names
  fn        the Function class of autograd_ops
  family    whose tolerance rule applies: "nn" (tests/test_nn_ops_edges_gpu.py), "conv" (rule A of tests/test_conv_edges_gpu.py),
            "roi" (tests/test_roi_edges_gpu.py)
  inputs    name -> host tensor, the tensor arguments of forward() (float32, or the integer type the kernel takes)
  diff      the differentiable inputs
  run       (A, T) -> output: the Function applied to the dict T of device tensors
  ref       the same operation with torch on the CPU in the dtype of the tensors it is given (float64: the reference, float32: torch's own
            evaluation for E32); conv / roi cases carry refs of their own form (conv_ref / roi_ref)
The shapes are the smallest at which the kernel form in question exists (taken from the edge suites of the kernels)."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import conv_refs as CR
import nn_refs as NR
import roi_refs as RR

EPS = 1e-5
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=gen(seed)) * scale + shift


# ---------------------------------------------------------------- presentations: host tensor -> the form handed to the Function
def base(t, device):
    """contiguous and 16-byte aligned"""
    return t.to(device).contiguous()


def every_other_column(t, device):
    """the same values as every other column of a buffer twice as wide: not contiguous"""
    buf = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=device)
    v = buf[..., ::2]
    v.copy_(t)
    return v


def transposed(t, device, d0=-2, d1=-1):
    """the same values as the transposed view of a buffer that holds them with dimensions d0 and d1 swapped: not contiguous"""
    buf = t.transpose(d0, d1).contiguous().to(device)
    return buf.transpose(d0, d1)


def transposed01(t, device):
    return transposed(t, device, 0, 1)


def offset(t, device):
    """a contiguous view one element into a larger buffer: data_ptr() % 16 == 4 (offset_view of tests/test_nn_ops_edges_gpu.py)"""
    from test_nn_ops_edges_gpu import offset_view
    return offset_view(t, device)


def stride0(value, shape, device):
    """the gradient y.sum().backward() hands over: one value expanded, every stride 0"""
    return torch.full((), value, dtype=torch.float32, device=device).expand(shape)


STRIDED = {"cols": every_other_column, "t": transposed, "t01": transposed01}


# ---------------------------------------------------------------- the table
class Case:
    def __init__(self, name, fn, family, inputs, diff, run, ref=None, loss=False, strided=None, refuses_strided=(), refuses_offset=(),
                 forms=None, chain=None, keep=None, conv_ref=None, roi_ref=None, K=None, env=None, bucket=(), restated=False,
                 forward_only=False, keeps_strides=(), no_strided=()):
        self.name, self.fn, self.family, self.inputs, self.diff, self.run, self.ref = name, fn, family, inputs, tuple(diff), run, ref
        self.loss = loss                        # the output is a 0-dim loss
        self.strided = strided or {}            # input -> key of STRIDED where "cols" does not apply
        self.refuses_strided = dict(refuses_strided) if not isinstance(refuses_strided, tuple) else {k: None for k in refuses_strided}
        self.refuses_offset = tuple(refuses_offset)     # inputs whose offset view the launcher refuses (ScdaNativeError): float4 only
        self.forms = forms                      # the form switch the device test asserts under an offset dy: "norm_up" (N.aligned16 /
                                                # SCDA_NO_NORM_UP_BWD_FUSION), "bn_join" (the aligned clone); conv-family cases
                                                # prove every launch with native.last_plan() instead
        self.chain = chain                      # (A, T) -> output of the chain of Functions the docstring promises bit equality with
        self.keep = keep                        # (p, seed): the reference needs T["keep"], read back from DropoutSeededFn on ones
        self.conv_ref, self.roi_ref, self.K = conv_ref, roi_ref, K
        self.env = env or {}                    # environment of the run
        self.bucket = tuple(bucket)             # parameters that may live in a scda_amd.flat bucket (presentation f)
        self.restated = restated                # the float64 reference is a restatement (gradcheck on the CPU), not torch's own op
        self.forward_only = forward_only
        self.keeps_strides = tuple(keeps_strides)       # inputs whose gradient is promised the input's strides
        self.no_strided = tuple(no_strided)     # inputs the run clones before the call: a strided form would never reach the Function

    def float_inputs(self):
        return [k for k, v in self.inputs.items() if v.dtype == torch.float32]

    def subsets(self):
        """every non-empty subset of the differentiable inputs"""
        return [s for n in range(1, len(self.diff) + 1) for s in itertools.combinations(self.diff, n)]

    def host(self, dtype, requires=None):
        """the inputs on the CPU with the float ones in dtype; `requires` (default: all of diff) as leaves that require grad"""
        requires = self.diff if requires is None else requires
        T = {}
        for k, v in self.inputs.items():
            T[k] = v.clone().to(dtype) if v.dtype == torch.float32 else v.clone()
            if k in requires:
                T[k].requires_grad_()
        return T

    def dy(self, out_shape):
        return randn(out_shape, 977) if not self.loss else None


def act_t(y, act, slope):
    return F.relu(y) if act == ACT_RELU else F.leaky_relu(y, slope) if act == ACT_LEAKY else y


# ---- conv family: bilinear cores; rule A needs the magnitude sum S of every output, which for a bilinear map is the same map (and its
# autograd gradients) on absolute operands
def bilinear_ref(core, act=ACT_NONE, slope=0.01, operands=("x", "w", "b")):
    """core(T) -> the pre-activation output.  -> conv_ref(case, dy, dtype) -> ({"y", operand...}, {S of each})"""
    def ref(case, dy, dtype):
        names = [k for k in operands if k in case.inputs]
        T = case.host(dtype, requires=names)
        pre = core(T)
        y = act_t(pre, act, slope)
        dyd = dy.to(dtype)
        grads = torch.autograd.grad(y, [T[k] for k in names], dyd, retain_graph=True)
        gpre = torch.autograd.grad(y, pre, dyd)[0].abs()          # |dy * act'|
        Tabs = {k: (v.detach().abs().requires_grad_() if k in names else v) for k, v in T.items()}
        Spre = core(Tabs)
        Sg = torch.autograd.grad(Spre, [Tabs[k] for k in names], gpre)
        vals = {"y": y.detach()}; S = {"y": Spre.detach()}
        for k, g, s in zip(names, grads, Sg):
            vals[k], S[k] = g.detach(), s.detach()
        return vals, S
    return ref


def conv_pool_ref(case, dy, dtype):
    """ConvPoolFn in the Winograd restatement of tests/conv_refs.py (S_w: the magnitude sums of the transform chain): relu(conv) ->
    2x2 max-pool; backward: the pool's scatter through the ReLU, then the layer's three gradients"""
    x, w, b = (case.inputs[k] for k in ("x", "w", "b"))
    full, Sfull = CR.wino_fwd(x, w, b, ACT_RELU, 0.0, dtype)
    y, idx = F.max_pool2d(full, 2, 2, return_indices=True)
    Sy = Sfull.flatten(2).gather(2, idx.flatten(2)).view_as(y)
    g = torch.zeros_like(full).flatten(2).scatter_(2, idx.flatten(2), torch.where(y > 0, dy.to(dtype), torch.zeros_like(y)).flatten(2)).view_as(full)
    dx, Sdx = CR.wino_dgrad(g, w, dtype=dtype)
    (dw, db), (Sw, Sb) = CR.wino_wgrad(g, x, dtype=dtype)
    return {"y": y, "x": dx, "w": dw, "b": db}, {"y": Sy, "x": Sdx, "w": Sw, "b": Sb}


def _conv_case(name, shape, cout, k, pad, act, slope, seed, env=None, bias=True):
    B, Cin, H, W = shape
    inputs = {"x": randn(shape, seed), "w": randn((cout, Cin, k, k), seed + 1, (Cin * k * k) ** -0.5), "b": randn((cout,), seed + 2)}
    if not bias:
        del inputs["b"]
    OH, OW = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    return Case(name, "Conv2dFn", "conv", inputs, tuple(inputs),
                run=lambda A, T: A.Conv2dFn.apply(T["x"], T["w"], T.get("b"), 1, pad, act, slope),
                conv_ref=bilinear_ref(lambda T: F.conv2d(T["x"], T["w"], T.get("b"), 1, pad), act, slope),
                K={"y": Cin * k * k + 1, "x": cout * k * k, "w": B * OH * OW + 1, "b": B * OH * OW + 1},
                env=env or {"SCDA_WINOGRAD": "0"}, bucket=("w", "b") if bias else ("w",), refuses_strided=("b",) if bias else ())


def _linear_case(bias=True):
    inputs = {"x": randn((3, 20), 21), "w": randn((7, 20), 22, 20 ** -0.5), "b": randn((7,), 23)}
    if not bias:
        del inputs["b"]
        return Case("linear[3x20->7,no bias]", "LinearFn", "conv", inputs, ("x", "w"),
                    run=lambda A, T: A.LinearFn.apply(T["x"], T["w"], None, ACT_NONE),
                    conv_ref=bilinear_ref(lambda T: F.linear(T["x"], T["w"])), K={"y": 21, "x": 7, "w": 4}, bucket=("w",))
    return Case("linear[3x20->7,relu]", "LinearFn", "conv", inputs, ("x", "w", "b"),
                run=lambda A, T: A.LinearFn.apply(T["x"], T["w"], T.get("b"), ACT_RELU),
                conv_ref=bilinear_ref(lambda T: F.linear(T["x"], T["w"], T.get("b")), ACT_RELU, 0.0),
                K={"y": 21, "x": 7, "w": 4, "b": 4}, bucket=("w", "b"), refuses_strided=("b",))


def _conv_pool_case():
    # the smallest layer native.conv_pool_fusable() serves: 8 tiles of 64 output rows x 25 blocks of 8 x 32 pixels = 200 tiles
    # Small integers, as rule B of tests/test_conv_edges_gpu.py: the 3.3 million values that are pooled are then exact in every
    # precision, so the ReLU masks and the winners of the 819 200 windows (exact ties: the first) are the reference's, and the
    # comparison of the gradients (a Gaussian dy) measures arithmetic, not which of two values 1e-7 apart a window picked.
    inputs = {"x": CR.ints((1, 32, 40, 160), -CR.INT_X, CR.INT_X, 31), "w": CR.ints((512, 32, 3, 3), -CR.INT_W, CR.INT_W, 32),
              "b": CR.ints((512,), -CR.INT_W, CR.INT_W, 33)}
    return Case("conv_pool[1x32x40x160->512]", "ConvPoolFn", "conv", inputs, ("x", "w", "b"),
                run=lambda A, T: A.ConvPoolFn.apply(T["x"], T["w"], T.get("b"), 0.0, None),
                conv_ref=conv_pool_ref, K={"y": 9 * 32 + 8, "x": 9 * 512 + 8, "w": 4 * 40 * 160 + 1, "b": 40 * 160 + 1}, bucket=("w", "b"),
                restated=True, refuses_strided=("w", "b"))


# ---- nn family
def _ew(name, fn, run, ref, seed=41, n_in=1, **kw):
    inputs = {("x" if n_in == 1 else "ab"[i]): randn((3, 85), seed + i, 2.0) for i in range(n_in)}
    return Case(name, fn, "nn", inputs, tuple(inputs), run, ref, **kw)


def _smooth_l1_ref(T):
    if T["pred"].dtype == torch.float64:
        return NR.smooth_l1_sum(T["pred"], T.get("mask"), T["target"], 3.0, 0.375)
    d = (T["pred"] * T["mask"] if "mask" in T else T["pred"]) - T["target"]
    near = (d.abs() < 1 / 9.).float()
    return (d.pow(2) * 9 / 2. * near + (d.abs() - 0.5 / 9.) * (1 - near)).sum() * 0.375


def _adv_inputs():
    C, n = 5, 33
    return {"x0": randn((C, n), 51, 2.0), "x1": randn((C, n), 52, 2.0), "t0": (torch.rand(1, n, generator=gen(53)) < 0.5).float(),
            "t1": (torch.rand(C, n, generator=gen(54)) < 0.5).float(), "w0": torch.rand(C, generator=gen(55))}


def _adv_ref(T):
    total = 0.0
    for x, t, w in ((T["x0"], T["t0"], T["w0"]), (T["x1"], T["t1"], None)):
        rows = F.binary_cross_entropy(torch.sigmoid(x), t.expand_as(x), reduction="none").mean(1)
        total = total + (rows * w if w is not None else rows).sum()
    return total * 0.375


def _ce_inputs():
    t = torch.tensor([0, 4, -1, 2, 2, -1, 1, 3, 0], dtype=torch.int64)
    return {"logits": randn((9, 5), 61, 3.0), "targets": t}


def _kp_inputs():
    t = torch.tensor([[5, -1, 62], [0, 31, -1]], dtype=torch.int32)
    return {"heat": randn((2, 3, 7, 9), 63, 2.0), "targets": t}


def _kp_ref(T):
    heat, t = T["heat"], T["targets"].reshape(-1).long()
    on = t >= 0
    x = heat.reshape(6, 63)
    return -torch.log_softmax(x[on], dim=1).gather(1, t[on][:, None]).sum() / int(on.sum())


def _inorm(T, act=ACT_NONE, slope=0.01):
    return act_t(F.instance_norm(T["x"], eps=EPS), act, slope)


def _drop(y, T, p):
    return torch.where(T["keep"], y * (1.0 / (1.0 - p)), torch.zeros_like(y))


def _up(y):
    return F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True)


def _bn_inputs(shape, seed):
    C = shape[1]
    return {"x": randn(shape, seed, 2.0, 0.3), "gamma": torch.rand(C, generator=gen(seed + 1)) + 0.5, "beta": randn((C,), seed + 2),
            "run_mean": randn((C,), seed + 3), "run_var": torch.rand(C, generator=gen(seed + 4)) + 0.5}


def _bn_train(T, act=ACT_NONE, slope=0.01):
    return act_t(F.batch_norm(T["x"], T["run_mean"].clone(), T["run_var"].clone(), T["gamma"], T["beta"], True, 0.1, EPS), act, slope)


P_DROP, SEED = 0.5, 0x0123456789ABCDE


def _roi_inputs():
    feat = randn((1, 4, 9, 11), 71)
    rois = torch.tensor([[0, 3.0, 5.0, 130.0, 90.0], [0, 40.5, 20.25, 60.0, 33.0], [0, 0.0, 0.0, 170.0, 140.0]], dtype=torch.float32)
    return {"features": feat, "rois": rois}


ROI_SCALE = 1.0 / 16.0


def _roi_align_ref(cm):
    def ref(case, dy):
        """the float64 statement of tests/roi_refs.py (with the per-pixel contribution count k and magnitude sum S of the gradient) and the
        C oracle's float32 forward, in the layout of the Function's output"""
        from oracle import native_ops as orc
        feat, rois = case.inputs["features"].numpy(), case.inputs["rois"].numpy()
        top = np.ascontiguousarray(dy.numpy().transpose(1, 0, 2, 3) if cm else dy.numpy())
        out, grad, k, S, _ = RR.roi_align(feat, rois, 3, 3, ROI_SCALE, top, stats=True)
        o32 = orc.roi_align_fwd(feat, rois, 3, 3, ROI_SCALE)
        if cm:
            out, o32 = out.transpose(1, 0, 2, 3), o32.transpose(1, 0, 2, 3)
        return dict(out64=out, out32=o32, grad64=grad, k=k, S=S)
    return ref


def _roi_pool_ref(case, dy):
    """bit for bit: the float32 restatement of the forward and the reference's backward rule on its argmax"""
    feat, rois = case.inputs["features"].numpy(), case.inputs["rois"].numpy()
    out, arg = RR.roi_pool_fwd(feat, rois, 2, 2, ROI_SCALE)
    return dict(out=out, grad=RR.roi_pool_bwd_reference_rule(dy.numpy(), arg, rois, feat.shape, 2, 2, ROI_SCALE))


def _cases():
    c = []
    c.append(_conv_case("conv[1x16x5x7->16,k3,leaky]", (1, 16, 5, 7), 16, 3, 1, ACT_LEAKY, 0.25, 11))
    c.append(_conv_case("conv[2x3x6x5->4,k1]", (2, 3, 6, 5), 4, 1, 0, ACT_NONE, 0.0, 15))
    c.append(_conv_case("conv[2x3x6x5->4,k1,no bias]", (2, 3, 6, 5), 4, 1, 0, ACT_NONE, 0.0, 18, bias=False))
    c.append(_conv_pool_case())
    c.append(_linear_case())
    c.append(_linear_case(bias=False))
    c.append(Case("maxpool2x2[2x3x7x9,relu_input]", "MaxPool2x2Fn", "nn", {"x": randn((2, 3, 7, 9), 82, 1.0, -0.7).clamp_min(0)}, ("x",),
                  run=lambda A, T: A.MaxPool2x2Fn.apply(T["x"], True), ref=lambda T: F.max_pool2d(F.relu(T["x"]), 2, 2)))
    c.append(Case("maxpool2x2[2x3x7x9]", "MaxPool2x2Fn", "nn", {"x": randn((2, 3, 7, 9), 81)}, ("x",),
                  run=lambda A, T: A.MaxPool2x2Fn.apply(T["x"]), ref=lambda T: F.max_pool2d(T["x"], 2, 2)))
    for mode, f in (("relu", F.relu), ("leaky", lambda v: F.leaky_relu(v, 0.01)), ("tanh", torch.tanh), ("sigmoid", torch.sigmoid)):
        c.append(_ew("act[%s]" % mode, "ActFn", (lambda m: lambda A, T: A.ActFn.apply(T["x"], A.N.ACT_MODE[m], 0.01))(mode),
                     (lambda g: lambda T: g(T["x"]))(f)))
    mask = (torch.rand(3, 85, generator=gen(83)) < 0.7).to(torch.uint8)
    c.append(Case("dropout[mask]", "DropoutFn", "nn", {"x": randn((3, 85), 84), "mask": mask}, ("x",),
                  run=lambda A, T: A.DropoutFn.apply(T["x"], T["mask"], 1.25), ref=lambda T: T["x"] * T["mask"].to(T["x"].dtype) * 1.25))
    c.append(Case("dropout[seeded]", "DropoutSeededFn", "nn", {"x": randn((3, 85), 85)}, ("x",), keep=(P_DROP, SEED),
                  run=lambda A, T: A.DropoutSeededFn.apply(T["x"], P_DROP, SEED, False), ref=lambda T: _drop(T["x"], T, P_DROP)))
    c.append(Case("dropout[seeded,relu_input]", "DropoutSeededFn", "nn", {"x": randn((3, 85), 86).clamp_min(0)}, ("x",), keep=(P_DROP, SEED),
                  run=lambda A, T: A.DropoutSeededFn.apply(T["x"], P_DROP, SEED, True), ref=lambda T: _drop(F.relu(T["x"]), T, P_DROP)))
    c.append(Case("adv_loss[2 groups,5x33]", "AdvLossFn", "nn", _adv_inputs(), ("x0", "x1"), loss=True,
                  run=lambda A, T: A.AdvLossFn.apply(0.375, 2, T["x0"], T["x1"], T["t0"], T["t1"], T["w0"], None), ref=_adv_ref,
                  refuses_strided=("w0",)))
    c.append(_ew("add", "AddFn", lambda A, T: A.AddFn.apply(T["a"], T["b"]), lambda T: T["a"] + T["b"], n_in=2, seed=87))
    c.append(_ew("add_relu", "AddReluFn", lambda A, T: A.AddReluFn.apply(T["a"], T["b"]), lambda T: F.relu(T["a"] + T["b"]), n_in=2, seed=89))
    c.append(Case("maxpool3x3s2[2x3x7x9]", "MaxPool3x3s2Fn", "nn", {"x": randn((2, 3, 7, 9), 91)}, ("x",), forward_only=True,
                  run=lambda A, T: A.MaxPool3x3s2Fn.apply(T["x"]), ref=lambda T: F.max_pool2d(T["x"], 3, 2, 1)))
    c.append(Case("roi_pool[1x4x9x11,3 rois]", "RoIPoolFn", "roi", _roi_inputs(), ("features",), roi_ref=_roi_pool_ref,
                  run=lambda A, T: A.RoIPoolFn.apply(T["features"], T["rois"], 2, 2, ROI_SCALE),
                  refuses_strided={"features": AssertionError, "rois": AssertionError}))
    for cm in (False, True):
        c.append(Case("roi_align[1x4x9x11,3 rois,%s]" % ("channel-major" if cm else "roi-major"), "RoIAlignFn", "roi", _roi_inputs(),
                      ("features",), roi_ref=_roi_align_ref(cm),
                      run=(lambda m: lambda A, T: A.RoIAlignFn.apply(T["features"], T["rois"], 3, 3, ROI_SCALE, m))(cm),
                      refuses_strided={"features": AssertionError, "rois": AssertionError}))
    c.append(Case("avg2x2s1[2x3x5x9]", "Avg2x2S1Fn", "nn", {"x": randn((2, 3, 5, 9), 93)}, ("x",),
                  run=lambda A, T: A.Avg2x2S1Fn.apply(T["x"]), ref=lambda T: F.avg_pool2d(T["x"], 2, 1)))
    c.append(Case("cross_entropy[9x5]", "SoftmaxCEFn", "nn", _ce_inputs(), ("logits",), loss=True,
                  run=lambda A, T: A.SoftmaxCEFn.apply(T["logits"], T["targets"], -1),
                  ref=lambda T: F.cross_entropy(T["logits"], T["targets"], ignore_index=-1)))
    c.append(Case("keypoint_ce[2x3x7x9]", "KeypointCEFn", "nn", _kp_inputs(), ("heat",), loss=True, strided={"heat": "t01"},
                  run=lambda A, T: A.KeypointCEFn.apply(T["heat"], T["targets"]), ref=_kp_ref, refuses_strided=("targets",),
                  keeps_strides=("heat",), restated=True))
    sl = {"pred": randn((6, 8), 95), "mask": (torch.rand(6, 8, generator=gen(96)) < 0.5).float(), "target": randn((6, 8), 97, 0.5)}
    c.append(Case("smooth_l1[6x8]", "SmoothL1Fn", "nn", sl, ("pred",), loss=True, restated=True,
                  run=lambda A, T: A.SmoothL1Fn.apply(T["pred"], T["mask"], T["target"], 3.0, 0.375), ref=_smooth_l1_ref))
    c.append(Case("smooth_l1[6x8,no mask]", "SmoothL1Fn", "nn", {k: v for k, v in sl.items() if k != "mask"}, ("pred",), loss=True, restated=True,
                  run=lambda A, T: A.SmoothL1Fn.apply(T["pred"], None, T["target"], 3.0, 0.375), ref=_smooth_l1_ref))
    for shape, form in (((2, 3, 7, 7), "HW=49"), ((1, 2, 64, 64), "HW=4096")):
        c.append(Case("instnorm[%s,leaky]" % form, "InstanceNormFn", "nn", {"x": randn(shape, 101, 2.0, 0.5)}, ("x",),
                      run=lambda A, T: A.InstanceNormFn.apply(T["x"], EPS, ACT_LEAKY, 0.01), ref=lambda T: _inorm(T, ACT_LEAKY, 0.01)))
        c.append(Case("instnorm_drop_add[%s]" % form, "InstNormDropAddFn", "nn", {"x": randn(shape, 103, 2.0, 0.5), "residual": randn(shape, 104)},
                      ("x", "residual"), keep=(P_DROP, SEED), restated=True,
                      run=lambda A, T: A.InstNormDropAddFn.apply(T["x"], T["residual"], EPS, P_DROP, SEED),
                      chain=lambda A, T: A.AddFn.apply(T["residual"], A.DropoutSeededFn.apply(A.InstanceNormFn.apply(T["x"], EPS, ACT_NONE, 0.01),
                                                                                             P_DROP, SEED, False)),
                      ref=lambda T: T["residual"] + _drop(_inorm(T), T, P_DROP)))
    up = (1, 2, 32, 128)
    c.append(Case("instnorm_up[1x2x32x128,relu]", "InstanceNormUpFn", "nn", {"x": randn(up, 105, 2.0, 0.5)}, ("x",), refuses_offset=("x",),
                  run=lambda A, T: A.InstanceNormUpFn.apply(T["x"], EPS, ACT_RELU, 0.0), forms="norm_up",
                  chain=lambda A, T: A.Upsample2xFn.apply(A.InstanceNormFn.apply(T["x"], EPS, ACT_RELU, 0.0)),
                  ref=lambda T: _up(_inorm(T, ACT_RELU, 0.0))))
    c.append(Case("instnorm_drop_add_up[1x2x32x128]", "InstNormDropAddUpFn", "nn", {"x": randn(up, 107, 2.0, 0.5), "residual": randn(up, 108)},
                  ("x", "residual"), keep=(P_DROP, SEED), refuses_offset=("x", "residual"), forms="norm_up", restated=True,
                  run=lambda A, T: A.InstNormDropAddUpFn.apply(T["x"], T["residual"], EPS, P_DROP, SEED),
                  chain=lambda A, T: A.Upsample2xFn.apply(A.InstNormDropAddFn.apply(T["x"], T["residual"], EPS, P_DROP, SEED)),
                  ref=lambda T: _up(T["residual"] + _drop(_inorm(T), T, P_DROP))))
    for shape in ((1, 4, 8, 8), (3, 4, 5, 5)):
        c.append(Case("batchnorm_train[%s,leaky]" % "x".join(map(str, shape)), "BatchNormTrainFn", "nn", _bn_inputs(shape, 111),
                      ("x", "gamma", "beta"), bucket=("gamma", "beta"), refuses_strided=("gamma", "beta"),
                      no_strided=("run_mean", "run_var"),       # (every run updates a fresh clone: batchnorm_fwd refuses strided ones)
                      run=lambda A, T: A.BatchNormTrainFn.apply(T["x"], T["gamma"], T["beta"], T["run_mean"].clone(), T["run_var"].clone(),
                                                                EPS, 0.1, ACT_LEAKY, 0.01),
                      ref=lambda T: _bn_train(T, ACT_LEAKY, 0.01)))
    j = _bn_inputs((1, 8, 7, 8), 121)
    j = {"x": j["x"], "residual": randn((1, 8, 7, 8), 126), **{k: v for k, v in j.items() if k != "x"}}
    c.append(Case("batchnorm_add_relu[1x8x7x8]", "BatchNormAddReluFn", "nn", j, ("x", "residual", "gamma", "beta"), bucket=("gamma", "beta"),
                  refuses_strided=("gamma", "beta"), refuses_offset=("x", "residual"), forms="bn_join", no_strided=("run_mean", "run_var"),
                  run=lambda A, T: A.BatchNormAddReluFn.apply(T["x"], T["residual"], T["gamma"], T["beta"], T["run_mean"].clone(),
                                                              T["run_var"].clone(), EPS, 0.1),
                  chain=lambda A, T: A.AddReluFn.apply(A.BatchNormTrainFn.apply(T["x"], T["gamma"], T["beta"], T["run_mean"].clone(),
                                                                                T["run_var"].clone(), EPS, 0.1, ACT_NONE, 0.0), T["residual"]),
                  ref=lambda T: F.relu(_bn_train(T) + T["residual"])))
    c.append(Case("batchnorm_eval[2x3x4x5,relu]", "BatchNormEvalFn", "nn", _bn_inputs((2, 3, 4, 5), 131), ("x",),
                  refuses_strided=("gamma", "beta", "run_mean", "run_var"),
                  run=lambda A, T: A.BatchNormEvalFn.apply(T["x"], T["gamma"], T["beta"], T["run_mean"], T["run_var"], EPS, ACT_RELU, 0.0),
                  ref=lambda T: F.relu(F.batch_norm(T["x"], T["run_mean"], T["run_var"], T["gamma"], T["beta"], False, 0.1, EPS))))
    for shape in ((2, 3, 5, 6), (1, 2, 8, 8)):        # (1, 2, 8, 8): the backward's rows kernel (IH % 8 == 0, an aligned dy)
        c.append(Case("upsample2x[%s]" % "x".join(map(str, shape)), "Upsample2xFn", "nn", {"x": randn(shape, 141)}, ("x",),
                      run=lambda A, T: A.Upsample2xFn.apply(T["x"]), ref=lambda T: _up(T["x"])))
    bp = {"p": torch.rand(3, 85, generator=gen(151)).clamp(1e-3, 1 - 1e-3), "t": torch.rand(3, 85, generator=gen(152))}
    c.append(Case("bce[3x85]", "BCEFn", "nn", bp, ("p",), loss=True, run=lambda A, T: A.BCEFn.apply(T["p"], T["t"]),
                  ref=lambda T: F.binary_cross_entropy(T["p"], T["t"])))
    c.append(Case("gap[2x5x7x7]", "GlobalAvgPoolFn", "nn", {"x": randn((2, 5, 7, 7), 161, 1.0, 0.5)}, ("x",),
                  run=lambda A, T: A.GlobalAvgPoolFn.apply(T["x"]), ref=lambda T: F.adaptive_avg_pool2d(T["x"], 1).flatten(1)))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
def functions_of(module):
    """every torch.autograd.Function subclass defined in a module"""
    return {n: o for n, o in vars(module).items()
            if isinstance(o, type) and issubclass(o, torch.autograd.Function) and o is not torch.autograd.Function and o.__module__ == module.__name__}


# ---------------------------------------------------------------- modules (scda_amd.layers): name, constructor, input shape
MODULES = [
    ("Conv2d[16->16,k3]", lambda L: L.Conv2d(16, 16, 3, padding=1), (1, 16, 5, 7), "conv", {"SCDA_WINOGRAD": "0"}),
    ("Conv2d[16->16,k3,fused leaky]", lambda L: L.Conv2d(16, 16, 3, padding=1, fused_act=ACT_LEAKY, slope=0.25), (1, 16, 5, 7), "conv",
     {"SCDA_WINOGRAD": "0"}),
    ("Conv2d[16->16,k3,row_period 7]", lambda L: _with(L.Conv2d(16, 16, 3, padding=1), row_period=7), (1, 16, 14, 7), "conv",
     {"SCDA_WINOGRAD": "0"}),
    ("ConvTranspose1x1[16->4]", lambda L: L.ConvTranspose1x1(16, 4), (2, 16, 3, 5), "conv", {}),
    ("ConvTranspose2x2s2[16->4]", lambda L: L.ConvTranspose2x2s2(16, 4), (2, 16, 3, 5), "conv", {}),
    ("ConvTranspose2x2s2[16->4,fused relu]", lambda L: L.ConvTranspose2x2s2(16, 4, fused_act=ACT_RELU), (2, 16, 3, 5), "conv", {}),
    ("Linear[20->7]", lambda L: L.Linear(20, 7), (3, 20), "conv", {}),
    ("InstanceNorm2d[relu]", lambda L: L.InstanceNorm2d(3, fused_act=ACT_RELU), (2, 3, 7, 7), "nn", {}),
    ("Upsample2x", lambda L: L.Upsample2x(), (2, 3, 5, 6), "nn", {}),
    ("BatchNorm2d[train]", lambda L: L.BatchNorm2d(4).train(), (3, 4, 5, 5), "nn", {}),
    ("BatchNorm2d[eval]", lambda L: L.BatchNorm2d(4).eval(), (3, 4, 5, 5), "nn", {}),
    ("BatchNorm2d.forward_add_relu[train]", lambda L: L.BatchNorm2d(8).train(), (1, 8, 7, 8), "nn", {}),
    ("BatchNorm2d.forward_add_relu[eval]", lambda L: L.BatchNorm2d(8).eval(), (1, 8, 7, 8), "nn", {}),
]


def _with(m, **attrs):
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def module_reference(name, m, T):
    """the module's operation with torch on the CPU in the dtype of T["x"]; m: the module (its configuration only), T: x (+ residual) and
    the parameters by their state_dict names"""
    x = T["x"]
    w, b = T.get("weight"), T.get("bias")
    if name.startswith("Conv2d"):
        rp = getattr(m, "row_period", 0)
        if rp:          # a vertical stack of independent maps of rp rows
            maps = x.reshape(x.shape[1], x.shape[2] // rp, rp, x.shape[3]).permute(1, 0, 2, 3)
            y = F.conv2d(maps, w, b, 1, 1)
            pre = y.permute(1, 0, 2, 3).reshape(1, y.shape[1], x.shape[2], x.shape[3])
        else:
            pre = F.conv2d(x, w, b, 1, 1)
        return pre, m.fused_act, m.slope
    if name.startswith("ConvTranspose1x1"):
        return F.conv_transpose2d(x, w, b), ACT_NONE, 0.0
    if name.startswith("ConvTranspose2x2s2"):
        return F.conv_transpose2d(x, w, b, stride=2), m.fused_act, m.slope
    if name.startswith("Linear"):
        return F.linear(x, w, b), ACT_NONE, 0.0
    if name.startswith("InstanceNorm2d"):
        return act_t(F.instance_norm(x, eps=m.eps), m.fused_act, m.slope)
    if name.startswith("Upsample2x"):
        return _up(x)
    rm, rv = T["running_mean"].clone(), T["running_var"].clone()
    y = F.batch_norm(x, rm, rv, w, b, m.training, m.momentum, m.eps)
    if "forward_add_relu" in name:
        return F.relu(y + T["residual"])
    return y


# ---------------------------------------------------------------- backward arity
def forward_arity(cls):
    """the number of arguments forward() takes behind ctx, or None where it takes *args (the call decides)"""
    import inspect
    params = list(inspect.signature(cls.forward).parameters.values())[1:]
    return None if any(p.kind == p.VAR_POSITIONAL for p in params) else len(params)


def static_backward_arity(cls):
    """the number of values every `return` of backward() lists, read from its source; None where a return builds its tuple at run time
    (or backward only raises): the device test counts what such a Function returns"""
    import ast
    import inspect
    import textwrap
    tree = ast.parse(textwrap.dedent(inspect.getsource(cls.backward)))
    counts = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Return):
            v = node.value
            if isinstance(v, ast.Tuple) and not any(isinstance(e, ast.Starred) for e in v.elts):
                counts.add(len(v.elts))
            elif isinstance(v, (ast.Call, ast.Name, ast.Attribute, ast.IfExp, ast.Subscript)):
                counts.add(1)
            else:
                return None
    return counts.pop() if len(counts) == 1 else None
