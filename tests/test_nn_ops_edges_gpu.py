"""The layer and loss kernels of scda_amd/csrc/nn_ops.hip at their edge shapes and values, against the fp64 restatements of
tests/nn_refs.py (checked on the CPU by tests/test_nn_refs.py).

Tolerance rule (every comparison that is not bit-exact): with ref64 the fp64 restatement evaluated on the fp32 inputs and torch32 the
same operation in fp32 with torch on the CPU (an independent implementation),
    E32 = max|torch32 - ref64| / max|ref64|,     max|kernel - ref64| / max|ref64| <= max(4 E32, 4 * 2^-23).
The factor 4 covers a different summation order and one or two ulp in the device's expf / logf / tanhf.  Each case prints
`EDGE <case> E32=... kernel=... bound=...` (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_refs as R

pytestmark = pytest.mark.gpu

ULP4 = 4.0 * 2.0 ** -23
SWEEP = 2048 * 4 * 256          # = 2 097 152 elements: one sweep of an element-wise launch (at most 2048 * 4 workgroups of 256)
SIZES = [1, 255, 257, SWEEP + 5]        # the last: a full sweep, then the grid-stride step into a second one with a tail of 5


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check(case, got, ref64, t32):
    """the tolerance rule; t32 = None where torch has no fp32 form of the case (E32 = 0)"""
    got, ref = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    assert torch.isfinite(ref).all(), case
    scale = ref.abs().max().item() or 1.0
    e32 = 0.0 if t32 is None else (t32.detach().cpu().double() - ref).abs().max().item() / scale
    err = (got - ref).abs().max().item() / scale
    bound = max(4.0 * e32, ULP4)
    print(f"\nEDGE {case} E32={e32:.3e} kernel={err:.3e} bound={bound:.3e}")      # (own line: pytest -s prints its dots unterminated)
    assert err <= bound, f"{case}: kernel error {err:.3e} over {bound:.3e} (E32 {e32:.3e})"


def same_bits_with_nan(got, want):
    """bit for bit, -inf and signed zeros included; NaN where and only where the other side has one"""
    got, want = got.detach().cpu(), want.detach().cpu()
    return (torch.equal(torch.isnan(got), torch.isnan(want))
            and torch.equal(bits(torch.nan_to_num(got, nan=0.0, posinf=float("inf"), neginf=float("-inf"))),
                            bits(torch.nan_to_num(want, nan=0.0, posinf=float("inf"), neginf=float("-inf")))))


def offset_view(t, device):
    """t on the device as a CONTIGUOUS view one element into a larger buffer: 4 bytes off every 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ---------------------------------------------------------------- element-wise
EDGE_VALUES = [100.0, -100.0, float("inf"), float("-inf"), -0.0]


def ew_input(n, seed, edges=True):
    x = torch.randn(n, generator=gen(seed)) * 3
    if edges:
        k = min(n, len(EDGE_VALUES))
        x[:k] = torch.tensor(EDGE_VALUES[:k])
        if n > 2 * len(EDGE_VALUES):
            x[-k:] = torch.tensor(EDGE_VALUES[:k])       # ... and in the tail of the last sweep
    return x


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode", ["relu", "leaky"])
def test_relu_leaky_bit_exact(cuda, mode, n):
    from scda_amd import native as N
    x = ew_input(n, 1); dy = ew_input(n, 2)
    zero = torch.zeros_like(x)
    y = N.act_fwd(x.to(cuda), N.ACT_MODE[mode], 0.01)
    want = torch.where(x > 0, x, zero if mode == "relu" else x * 0.01)
    assert torch.equal(bits(y), bits(want))
    dx = N.act_bwd(dy.to(cuda), y, N.ACT_MODE[mode], 0.01)
    assert torch.equal(bits(dx), bits(torch.where(want > 0, dy, zero if mode == "relu" else dy * 0.01)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode,fn", [("tanh", torch.tanh), ("sigmoid", torch.sigmoid)])
def test_tanh_sigmoid(cuda, mode, fn, n):
    from scda_amd import native as N
    x = ew_input(n, 3); dy = ew_input(n, 4, edges=False)
    y = N.act_fwd(x.to(cuda), N.ACT_MODE[mode], 0.0)
    check(f"act_fwd[{mode},n={n}]", y, R.act_fwd(x, mode), fn(x))
    yc = y.cpu()
    dx = N.act_bwd(dy.to(cuda), y, N.ACT_MODE[mode], 0.0)
    t32 = dy * (1 - yc * yc) if mode == "tanh" else dy * yc * (1 - yc)
    check(f"act_bwd[{mode},n={n}]", dx, R.act_bwd(dy, yc, mode), t32)


@pytest.mark.parametrize("n", SIZES)
def test_add_relu_axpby(cuda, n):
    from scda_amd import native as N
    a = ew_input(n, 5); b = ew_input(n, 6, edges=False)
    s = a + b
    assert torch.equal(bits(N.add_relu(a.to(cuda), b.to(cuda))), bits(torch.where(s > 0, s, torch.zeros_like(s))))
    a = ew_input(n, 7, edges=False)
    alpha, beta = 0.75, -1.5            # exact in fp32: the kernel's float arguments are the reference's numbers
    check(f"axpby[n={n}]", N.axpby(a.to(cuda), b.to(cuda), alpha, beta), R.axpby(a, b, alpha, beta), alpha * a + beta * b)
    check(f"axpby[no b,n={n}]", N.axpby(a.to(cuda), None, alpha, beta), R.axpby(a, None, alpha, beta), alpha * a)


@pytest.mark.parametrize("n", SIZES)
def test_dropout_forms_agree(cuda, n):
    from scda_amd import native as N
    p, seed = 0.3, 0x1234567890ABCDEF
    scale = 1.0 / (1.0 - p)
    x = ew_input(n, 8, edges=False)
    m = N.dropout_mask((n,), p, seed, cuda)
    y = N.dropout_apply(x.to(cuda), m, scale)
    assert torch.equal(bits(y), bits(torch.where(m.cpu().bool(), x * scale, torch.zeros_like(x))))
    assert torch.equal(bits(N.dropout_seeded(x.to(cuda), p, seed, scale)), bits(y))
    if n > 1 << 20:         # the index is the only input: the second sweep continues the sequence of a shorter call
        assert torch.equal(m[:1 << 20], N.dropout_mask((1 << 20,), p, seed, cuda))
        assert abs(m.float().mean().item() - 0.7) < 5 * (0.3 * 0.7 / n) ** 0.5


def test_dropout_p_edges(cuda):
    from scda_amd import native as N
    n = 1 << 20
    x = ew_input(n, 9, edges=False).to(cuda)
    assert N.dropout_mask((n,), 0.0, 77, cuda).all()
    assert torch.equal(bits(N.dropout_seeded(x, 0.0, 77, 1.0)), bits(x))
    kept = int(N.dropout_mask((n,), 0.999, 77, cuda).sum())
    sigma = (n * 0.001 * 0.999) ** 0.5
    print(f"\nEDGE dropout[p=0.999] kept={kept} expected={n * 0.001:.1f} sigma={sigma:.1f}")
    assert abs(kept - n * 0.001) <= 5 * sigma
    y = N.dropout_seeded(x, 0.999, 77, 1000.0)
    assert int((y != 0).sum()) == kept


# ------------------------------------------------------------------------ pools
@pytest.mark.parametrize("hw", [(7, 9), (8, 12)])
def test_maxpools_nan_and_inf(cuda, hw):
    from scda_amd import native as N
    x = R.pool_input((2, 3) + hw, 10)
    xr = x.clone().requires_grad_()
    yt = F.max_pool2d(xr, 2, 2)
    dy = torch.randn(yt.shape, generator=gen(11))
    yt.backward(dy)
    y, idx = N.maxpool2x2_fwd(x.to(cuda))
    assert torch.isnan(yt).sum() == 2 and (yt == float("-inf")).sum() >= 3
    assert torch.isnan(y).sum() == 2 and torch.equal(y.cpu() == float("-inf"), yt == float("-inf"))      # an all -inf window stays -inf
    assert same_bits_with_nan(y, yt)
    assert torch.equal(idx.cpu().long(), R.maxpool2x2(x)[1])
    assert torch.equal(bits(N.maxpool2x2_bwd(dy.to(cuda), idx, x.shape)), bits(xr.grad))
    y3, t3 = N.maxpool3x3s2_fwd(x.to(cuda)).cpu(), F.max_pool2d(x, 3, 2, 1)
    assert torch.isnan(t3).any() and (t3 == float("-inf")).any()
    assert torch.isnan(y3).any() and torch.equal(y3 == float("-inf"), t3 == float("-inf"))
    assert same_bits_with_nan(y3, t3)


@pytest.mark.parametrize("hw", [(7, 9), (8, 12)])
def test_maxpool_backward_with_relu_fused(cuda, hw):
    from scda_amd import native as N
    x = R.pool_input((4, 8) + hw, 12, edges=False).to(cuda)
    y, idx = N.maxpool2x2_fwd(x)
    zeros = (y == 0).float().mean().item()
    assert 0.2 < zeros < 0.45, zeros                    # about a third of the windows are all-zero ties
    assert (idx[y == 0] == 0).all()                     # ... and the first element wins them
    dy = torch.randn(y.shape, generator=gen(13)).to(cuda)
    fused = N.maxpool2x2_bwd(dy, idx, x.shape, relu_y=y)
    two = N.act_bwd(N.maxpool2x2_bwd(dy, idx, x.shape), x, N.ACT_MODE["relu"], 0.0)
    assert torch.equal(bits(fused), bits(two))
    assert (fused != 0).sum() == (y > 0).sum()


@pytest.mark.parametrize("shape", [(3, 5, 8, 8), (1, 2, 2, 2), (2, 3, 5, 9)])
def test_avg2x2s1(cuda, shape):
    from scda_amd import autograd_ops as A
    x = torch.randn(*shape, generator=gen(14))
    dy = torch.randn(shape[0], shape[1], shape[2] - 1, shape[3] - 1, generator=gen(15))
    x64 = x.double().requires_grad_(); R.avg2x2s1(x64).backward(dy.double())
    x32 = x.clone().requires_grad_(); y32 = F.avg_pool2d(x32, 2, 1); y32.backward(dy)
    xg = x.to(cuda).requires_grad_(); yg = A.Avg2x2S1Fn.apply(xg); yg.backward(dy.to(cuda))
    check(f"avg2x2s1_fwd{shape}", yg, R.avg2x2s1(x), y32)
    check(f"avg2x2s1_bwd{shape}", xg.grad, x64.grad, x32.grad)


# ------------------------------------------------------------------- reductions
@pytest.mark.parametrize("M,N_", [(1, 1), (7, 33), (8, 32), (9, 31), (513, 100), (512, 4096)])
def test_colsum(cuda, M, N_):
    from scda_amd import native as N
    x = torch.randn(M, N_, generator=gen(16)); pre = torch.randn(N_, generator=gen(17))
    check(f"colsum[{M}x{N_}]", N.colsum(x.to(cuda)), R.colsum(x), x.sum(0))
    out = pre.to(cuda)
    assert N.colsum(x.to(cuda), out=out) is out
    check(f"colsum[{M}x{N_},accumulate]", out, pre.double() + R.colsum(x), pre + x.sum(0))


# (B, C, HW): the 128-split cap (one slice, 128 slices), the scalar path across a slice boundary, float4 with a ragged last slice,
# many channels (nsplit 32), odd sizes, more channels than workgroups' worth (2048 / C < 1), one pixel
BIAS_SHAPES = [(1, 1, 2048), (1, 1, 262144), (2, 3, 2049), (2, 5, 2052), (1, 64, 4200), (3, 7, 8191), (1, 2500, 49), (4, 16, 1)]


@pytest.mark.parametrize("B,C,HW", BIAS_SHAPES)
def test_bias_grad_nchw(cuda, B, C, HW):
    from scda_amd import native as N
    x = torch.randn(B, C, HW, generator=gen(18)) + 0.1; pre = torch.randn(C, generator=gen(19))
    form = "vector" if HW % 4 == 0 else "scalar"
    check(f"bias_grad[{B},{C},{HW};{form}]", N.bias_grad_nchw(x.to(cuda)), R.bias_grad_nchw(x), x.sum((0, 2)))
    out = pre.to(cuda)
    N.bias_grad_nchw(x.to(cuda), out=out)
    check(f"bias_grad[{B},{C},{HW};{form},accumulate]", out, pre.double() + R.bias_grad_nchw(x), pre + x.sum((0, 2)))


def test_bias_grad_nchw_on_an_offset_view(cuda):
    """a contiguous view 4 bytes off a 16-byte boundary: the launcher must not choose the float4 loads"""
    from scda_amd import native as N
    x = torch.randn(1, 64, 4200, generator=gen(20)) + 0.1
    check("bias_grad[1,64,4200;offset view -> scalar]", N.bias_grad_nchw(offset_view(x, cuda)), R.bias_grad_nchw(x), x.sum((0, 2)))


# small (LDS-staged) form: HW <= 64 and >= 4096 planes -- a ragged last group of 256 planes; exactly 64 KB of LDS; one plane per
# workgroup below the switch
@pytest.mark.parametrize("shape,bwd", [((1, 4133, 7, 7), True), ((1, 4096, 8, 8), False), ((2, 2100, 1, 1), False), ((1, 4095, 7, 7), True)])
def test_gap(cuda, shape, bwd):
    from scda_amd import autograd_ops as A
    x = torch.randn(*shape, generator=gen(21)) + 0.5
    form = "small" if shape[2] * shape[3] <= 64 and shape[0] * shape[1] >= 4096 else "plain"
    xg = x.to(cuda).requires_grad_()
    yg = A.GlobalAvgPoolFn.apply(xg)
    check(f"gap_fwd{shape};{form}", yg, R.gap(x), F.adaptive_avg_pool2d(x, 1).flatten(1))
    if bwd:
        dy = torch.randn(shape[:2], generator=gen(22))
        x64 = x.double().requires_grad_(); R.gap(x64).backward(dy.double())
        x32 = x.clone().requires_grad_(); F.adaptive_avg_pool2d(x32, 1).flatten(1).backward(dy)
        yg.backward(dy.to(cuda))
        check(f"gap_bwd{shape}", xg.grad, x64.grad, x32.grad)


@pytest.mark.parametrize("C", [1, 255, 257, 5000])
def test_row_mean(cuda, C):
    from scda_amd import native as N
    x = torch.randn(3, C, generator=gen(23)) + 0.5
    check(f"row_mean[C={C}]", N.row_mean(x.to(cuda)), R.row_mean(x), x.mean(1))


# ----------------------------------------------------------------------- losses
CE_CASES = [(1, 1, 3, 1), (1, 5, 3, 1), (1025, 2, 3, None), (77, 5, 3, None), (77, 5, 1e4, None), (77, 5, 3, 1)]


@pytest.mark.parametrize("rows,classes,scale,keep", CE_CASES)
def test_cross_entropy(cuda, rows, classes, scale, keep):
    from scda_amd import autograd_ops as A
    x, t = R.ce_case(rows, classes, scale, keep)
    x64 = x.double().requires_grad_(); l64 = R.cross_entropy(x64, t, -1); (l64 * 0.375).backward()
    x32 = x.clone().requires_grad_(); l32 = F.cross_entropy(x32, t, ignore_index=-1); (l32 * 0.375).backward()
    xg = x.to(cuda).requires_grad_(); lg = A.cross_entropy(xg, t.to(cuda), -1); (lg * 0.375).backward()
    case = f"[{rows}x{classes},scale={scale:g},valid={'some' if keep is None else keep}]"
    check("cross_entropy" + case, lg.reshape(1), l64.reshape(1), l32.reshape(1))
    check("cross_entropy_grad" + case, xg.grad, x64.grad, x32.grad)
    assert not xg.grad[t.to(cuda) == -1].any()


def test_cross_entropy_every_row_ignored(cuda):
    from scda_amd import autograd_ops as A
    x, t = R.ce_case(77, 5, 3, 0)
    assert (t == -1).all() and torch.isnan(F.cross_entropy(x, t, ignore_index=-1)) and torch.isnan(R.cross_entropy(x.double(), t, -1))
    xg = x.to(cuda).requires_grad_()
    lg = A.cross_entropy(xg, t.to(cuda), -1)
    lg.backward()
    assert torch.isnan(lg)
    assert torch.equal(bits(xg.grad), torch.zeros(77, 5, dtype=torch.int32))


def test_row_softmax_and_accuracy_edges(cuda):
    from scda_amd import native as N
    for rows, classes, scale, keep in CE_CASES:
        x, t = R.ce_case(rows, classes, scale, keep)
        case = f"[{rows}x{classes},scale={scale:g}]"
        check("row_softmax" + case, N.row_softmax(x.to(cuda)), R.row_softmax(x), F.softmax(x, 1))
        v = t != -1
        check("accuracy" + case, N.accuracy(x.to(cuda), t.to(cuda), -1), R.accuracy(x, t, -1).reshape(1),
              ((x[v].argmax(1) == t[v]).float().mean() * 100).reshape(1))
    for t in (torch.tensor([0, 1, 0, 1]), torch.tensor([1, 2, 2, 1]), torch.tensor([0, -1, 1, 1])):     # exact ties: the first maximum
        v = t != -1
        want = (R.TIES[v].argmax(1) == t[v]).float().mean() * 100
        if v.all():                     # (4 rows: every figure is exact)
            assert R.accuracy(R.TIES, t, -1).item() == want.item() and N.accuracy(R.TIES.to(cuda), t.to(cuda), -1).item() == want.item()
        check(f"accuracy[ties,{t.tolist()}]", N.accuracy(R.TIES.to(cuda), t.to(cuda), -1), R.accuracy(R.TIES, t, -1).reshape(1), want.reshape(1))
    t = torch.full((4,), -1, dtype=torch.int64)
    assert torch.isnan(torch.empty(0).mean()) and torch.isnan(N.accuracy(R.TIES.to(cuda), t.to(cuda), -1)).all()


def smooth_l1_planted():
    """(pred, target) pairs with pred * 1 - target exactly 0, +-1/9 as fp32 rounds it and one ulp either side; (branch, gradient)"""
    thr = np.float32(1.0) / np.float32(9.0)
    lo, hi = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    nine = np.float32(9.0)
    rows = [(0.375, 0.375, "quad", 0.0)]
    for d, branch in ((lo, "quad"), (thr, "linear"), (hi, "linear")):
        for s in (1.0, -1.0):
            rows.append((s * float(d), 0.0, branch, s * float(np.float32(d) * nine) if branch == "quad" else s))
    assert float(lo * nine) == 1.0 - 2.0 ** -24 and float(np.float32(hi * nine)) != 1.0       # the two branches differ there in fp32
    return rows


@pytest.mark.parametrize("with_mask", [True, False])
def test_smooth_l1(cuda, with_mask):
    from scda_amd import autograd_ops as A
    n = 2 * 131072 + 3              # the forward's 512 workgroups cover 131 072 elements a sweep: two sweeps and a tail
    p = torch.randn(n, generator=gen(24)); t = torch.randn(n, generator=gen(25)) * 0.5
    m = (torch.rand(n, generator=gen(26)) < 0.3).float() if with_mask else None
    rows = smooth_l1_planted()
    where = list(range(len(rows))) + [n - 1 - i for i in range(len(rows))]          # first sweep and the tail
    for j, i in enumerate(where):
        p[i], t[i] = rows[j % len(rows)][:2]
        if with_mask:
            m[i] = 1.0
    p64 = p.double().requires_grad_(); l64 = R.smooth_l1_sum(p64, m, t, 3.0); l64.backward()
    p32 = p.clone().requires_grad_()
    d = (p32 * m if with_mask else p32) - t
    near = (d.abs() < 1 / 9.).float()
    l32 = (d.pow(2) * 9 / 2. * near + (d.abs() - 0.5 / 9.) * (1 - near)).sum(); l32.backward()
    pg = p.to(cuda).requires_grad_()
    lg = A.smooth_l1_sum(pg, m.to(cuda) if with_mask else None, t.to(cuda), 3.0, 1.0); lg.backward()
    quad = R.smooth_l1_branch(p, m, t, 3.0)
    g = pg.grad.cpu()
    for j, i in enumerate(where):       # upstream gradient 1, scale 1: the element's gradient IS the branch's derivative
        _, _, branch, want = rows[j % len(rows)]
        assert bool(quad[i]) == (branch == "quad"), (i, branch)
        assert g[i].item() == want and p64.grad[i].item() == want, (i, branch, g[i].item(), p64.grad[i].item(), want)
    check(f"smooth_l1[mask={with_mask}]", lg.reshape(1), l64.reshape(1), l32.reshape(1))
    check(f"smooth_l1_grad[mask={with_mask}]", pg.grad, p64.grad, p32.grad)


def test_bce_with_the_clamped_elements(cuda):
    from scda_amd import autograd_ops as A
    p = torch.rand(1, 1024, generator=gen(23)).clamp(1e-6, 1 - 1e-6); p[0, 0] = 0.0; p[0, 1] = 1.0
    t = torch.rand(1, 1024, generator=gen(24))
    p64 = p.double().requires_grad_(); l64 = R.bce(p64, t); (l64 * 1.75).backward()
    p32 = p.clone().requires_grad_(); l32 = F.binary_cross_entropy(p32, t); (l32 * 1.75).backward()
    pg = p.to(cuda).requires_grad_(); lg = A.binary_cross_entropy(pg, t.to(cuda)); (lg * 1.75).backward()
    check("bce", lg.reshape(1), l64.reshape(1), l32.reshape(1))
    check("bce_grad", pg.grad, p64.grad, p32.grad)
    check("bce_grad[interior]", pg.grad[:, 2:], p64.grad[:, 2:], p32.grad[:, 2:])
    g = pg.grad.cpu().double()
    for i in (0, 1):                    # the whole 1e-12 clamp path, each element on its own
        want = 1.75 * (p[0, i].double() - t[0, i].double()) / 1e-12 / 1024
        assert p64.grad[0, i].item() == pytest.approx(want.item(), rel=1e-14)
        rel = abs(g[0, i].item() - want.item()) / abs(want.item())
        print(f"\nEDGE bce_grad[p={p[0, i].item():g}] kernel={rel:.3e} bound={ULP4:.3e}")
        assert rel <= ULP4


@pytest.mark.parametrize("n", [1, 1023, 1025])
@pytest.mark.parametrize("C", [1, 5])
def test_adversarial_loss(cuda, C, n):
    """sigmoid_bce_rows through adversarial_loss: two groups accumulate into one scalar"""
    from scda_amd import autograd_ops as A
    xs, g64, g32, gg = [], [], [], []
    l32 = 0.0
    for k in range(2):
        x = torch.randn(C, n, generator=gen(27 + k)) * 3
        t = (torch.rand(1 if k == 0 else C, n, generator=gen(29 + k)) < 0.5).float()
        x[0, 0] = 100.0; t[0, 0] = 0.0                  # both logs at their clamp
        if n > 1:
            x[0, 1] = -100.0; x[-1, -1] = -100.0; t[0, 1] = 1.0
        w = torch.rand(C, generator=gen(31 + k))
        if C > 1:
            w[0] = 0.0
        w = w if k == 0 or C > 1 else None
        xs.append(x)
        x64 = x.double().requires_grad_(); g64.append((x64, t, w))
        x32 = x.clone().requires_grad_(); g32.append(x32)
        xg = x.to(cuda).requires_grad_(); gg.append((xg, t.to(cuda), w.to(cuda) if w is not None else None))
        for c in range(C):
            l32 = l32 + (w[c] if w is not None else 1.0) * F.binary_cross_entropy(torch.sigmoid(x32[c]), t[c if k else 0])
    l64 = R.adversarial_loss(g64, 0.375); l64.backward()
    (l32 * 0.375).backward()
    lg = A.adversarial_loss(gg, 0.375); lg.backward()
    check(f"adversarial_loss[C={C},n={n}]", lg.reshape(1), l64.reshape(1), (l32 * 0.375).reshape(1))
    for k in range(2):
        check(f"adversarial_loss_grad[C={C},n={n},group {k}]", gg[k][0].grad, g64[k][0].grad, g32[k].grad)
    for k in range(2):      # the clamped logits on their own: sigmoid'(+-100) is 0 in fp32, so is the gradient, exactly (the fp64
        g = gg[k][0].grad   # restatement keeps 1e-32 there, which makes E32 = 1 and the rule vacuous for C = 1, n = 1)
        assert g[0, 0].item() == 0.0 and (n == 1 or (g[0, 1].item() == 0.0 and g[-1, -1].item() == 0.0))
    if C == 5:
        assert not gg[0][0].grad[0].any()               # weight 0


# ------------------------------------------------------------------------ norms
ACT_FN = [lambda v: v, F.relu, lambda v: F.leaky_relu(v, 0.01)]
EPS = 1e-5


def inorm_all(cuda, case, x, dy, act, expect_t32=True, place=None):
    """forward and backward of one instance-norm case through its autograd wrapper against the rule; place: how x gets to the device"""
    from scda_amd import autograd_ops as A
    x64 = x.double().requires_grad_(); y64, _, _ = R.instance_norm(x64, EPS, act, 0.01); y64.backward(dy.double())
    y32 = g32 = None
    if expect_t32:
        x32 = x.clone().requires_grad_(); y32 = ACT_FN[act](F.instance_norm(x32, eps=EPS)); y32.backward(dy); g32 = x32.grad
    xg = (place(x) if place else x.to(cuda)).detach().requires_grad_()
    yg = A.InstanceNormFn.apply(xg, EPS, act, 0.01); yg.backward(dy.to(cuda))
    check(f"instnorm_fwd[{case},act={act}]", yg, y64, y32)
    check(f"instnorm_bwd[{case},act={act}]", xg.grad, x64.grad, g32)
    return yg, xg.grad


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (31, 33), (25, 41)])         # HW = 1, 49, 1023, 1025: the generic kernel
def test_instance_norm_plane_sizes(cuda, hw, act):
    from scda_amd import native as N
    x = torch.randn(2, 3, *hw, generator=gen(33)) * 2 + 0.5
    dy = torch.randn(2, 3, *hw, generator=gen(34))
    inorm_all(cuda, f"HW={hw[0] * hw[1]}", x, dy, act, expect_t32=hw != (1, 1))
    # a constant plane (2.5: its sums are exact, so the mean is): output 0, rstd = 1 / sqrt(eps), a finite gradient
    c = torch.full((1, 1) + hw, 2.5)
    yg, dxg = inorm_all(cuda, f"HW={hw[0] * hw[1]},constant", c, dy[:1, :1], act, expect_t32=False)
    assert not yg.any() and torch.isfinite(dxg).all()
    _, mean, rstd = N.instnorm_fwd(c.to(cuda), EPS, act, 0.01)
    assert mean.item() == 2.5 and abs(rstd.item() * np.sqrt(np.float64(np.float32(EPS))) - 1.0) <= ULP4
    # mean 1e3, std 1e-2: two-pass statistics hold where E[x^2] - mean^2 would not
    if hw != (1, 1):
        ill = (1e3 + 1e-2 * torch.randn(1, 1, *hw, generator=gen(35)))
        inorm_all(cuda, f"HW={hw[0] * hw[1]},mean 1e3 std 1e-2", ill, dy[:1, :1], act)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_instance_norm_4096_aligned_and_offset(cuda, act):
    """HW = 4096: the register-resident float4 kernel on an aligned tensor, the generic one on a view 4 bytes off"""
    x = torch.randn(2, 3, 64, 64, generator=gen(36)) * 2 + 0.5
    dy = torch.randn(2, 3, 64, 64, generator=gen(37))
    off = lambda t: offset_view(t, cuda)
    assert x.to(cuda).data_ptr() % 16 == 0
    inorm_all(cuda, "HW=4096,aligned;register", x, dy, act)
    inorm_all(cuda, "HW=4096,offset view;generic", x, dy, act, place=off)
    ill = 1e3 + 1e-2 * torch.randn(1, 2, 64, 64, generator=gen(38))
    inorm_all(cuda, "HW=4096,aligned;register,mean 1e3 std 1e-2", ill, dy[:1, :2], act)
    inorm_all(cuda, "HW=4096,offset view;generic,mean 1e3 std 1e-2", ill, dy[:1, :2], act, place=off)


def drop_add_refs(x, res, dy, keep, p):
    x64 = x.double().requires_grad_()
    y64, m64, r64 = R.instnorm_drop_add(x64, res.double(), keep, EPS, p); y64.backward(dy.double())
    x32 = x.clone().requires_grad_()
    y32 = res + torch.where(keep, F.instance_norm(x32, eps=EPS) * (1.0 / (1.0 - p)), torch.zeros_like(x)); y32.backward(dy)
    return (y64, x64.grad, m64, r64), (y32, x32.grad)


def test_instnorm_drop_add_aligned_offset_and_device_seed(cuda):
    from scda_amd import native as N
    p, seed = 0.5, 0x0123456789ABCDE
    x = torch.randn(2, 3, 64, 64, generator=gen(39)) * 2 + 0.5
    res = torch.randn(2, 3, 64, 64, generator=gen(40)); dy = torch.randn(2, 3, 64, 64, generator=gen(41))
    keep = N.dropout_mask(tuple(x.shape), p, seed, cuda).cpu().bool()        # keep(i) is a function of (seed, flat index) alone
    (y64, dx64, m64, r64), (y32, dx32) = drop_add_refs(x, res, dy, keep, p)
    outs = {}
    for form, xg in (("aligned;register", x.to(cuda)), ("offset view;generic", offset_view(x, cuda))):
        y, mean, rstd = N.instnorm_drop_add_fwd(xg, res.to(cuda), EPS, p, seed)
        dx = N.instnorm_drop_bwd(dy.to(cuda), xg, mean, rstd, p, seed)
        check(f"instnorm_drop_add_fwd[{form}]", y, y64, y32)
        check(f"instnorm_drop_bwd[{form}]", dx, dx64, dx32)
        check(f"instnorm_drop_add_fwd mean[{form}]", mean, m64, x.mean((2, 3)).reshape(-1))
        check(f"instnorm_drop_add_fwd rstd[{form}]", rstd, r64, (x.var((2, 3), unbiased=False) + EPS).rsqrt().reshape(-1))
        outs[form] = (y, mean, rstd, dx)
        assert torch.equal((y.cpu() != res), keep)          # the kept / dropped pattern (no normalised value is exactly 0 here)
    a, o = outs["aligned;register"], outs["offset view;generic"]
    assert torch.equal(a[0] != res.to(cuda), o[0] != res.to(cuda))
    # the seed in device memory (what a recorded graph uses: autograd_ops passes the tensor through, native switches on it)
    seed_dev = torch.tensor([seed], dtype=torch.int64, device=cuda)
    for form, xg in (("aligned", x.to(cuda)), ("offset", offset_view(x, cuda))):
        ref = outs["aligned;register" if form == "aligned" else "offset view;generic"]
        y, mean, rstd = N.instnorm_drop_add_fwd(xg, res.to(cuda), EPS, p, seed_dev)
        dx = N.instnorm_drop_bwd(dy.to(cuda), xg, mean, rstd, p, seed_dev)
        for got, want in zip((y, mean, rstd, dx), ref):
            assert torch.equal(bits(got), bits(want)), form


def bn_case(shape, seed):
    C = shape[1]
    # two values per channel: dx is O(eps / var) -- a spread of 1e-2 keeps eps in play instead of comparing two roundings of ~0
    x = torch.randn(*shape, generator=gen(seed)) * (0.01 if shape[0] * shape[2] * shape[3] == 2 else 2.0) + 0.3
    return (x, torch.rand(C, generator=gen(seed + 1)) + 0.5, torch.randn(C, generator=gen(seed + 2)), torch.randn(C, generator=gen(seed + 3)),
            torch.rand(C, generator=gen(seed + 4)) + 0.5, torch.randn(*shape, generator=gen(seed + 5)))


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (4, 10, 8, 8), (1, 4, 1, 4)])      # (1, 4, 1, 4): batch 1 = the plane kernels
def test_batch_norm_train(cuda, shape, act):
    from scda_amd import autograd_ops as A, native as N
    x, g, b, rm0, rv0, dy = bn_case(shape, 42)
    x64, g64, b64 = (v.double().requires_grad_() for v in (x, g, b))
    y64, rm64, rv64, _, _ = R.batch_norm_train(x64, g64, b64, rm0, rv0, EPS, 0.1, act, 0.01); y64.backward(dy.double())
    x32, g32, b32 = (v.clone().requires_grad_() for v in (x, g, b))
    rm32, rv32 = rm0.clone(), rv0.clone()
    y32 = ACT_FN[act](F.batch_norm(x32, rm32, rv32, g32, b32, True, 0.1, EPS)); y32.backward(dy)
    xg, gg, bg = (v.to(cuda).requires_grad_() for v in (x, g, b))
    rmg, rvg = rm0.to(cuda), rv0.to(cuda)
    yg = A.BatchNormTrainFn.apply(xg, gg, bg, rmg, rvg, EPS, 0.1, act, 0.01); yg.backward(dy.to(cuda))
    case = f"[{shape},act={act}]"
    check("batchnorm_fwd" + case, yg, y64, y32)
    check("batchnorm_bwd dx" + case, xg.grad, x64.grad, x32.grad)
    check("batchnorm_bwd dgamma" + case, gg.grad, g64.grad, g32.grad)
    check("batchnorm_bwd dbeta" + case, bg.grad, b64.grad, b32.grad)
    check("batchnorm running_mean" + case, rmg, rm64, rm32)
    check("batchnorm running_var" + case, rvg, rv64, rv32)
    # the unbiased factor on its own: momentum 1 leaves running_var = var * n / (n - 1), whatever var's size
    n = shape[0] * shape[2] * shape[3]
    rm1, rv1 = torch.zeros(shape[1], device=cuda), torch.zeros(shape[1], device=cuda)
    N.batchnorm_fwd(xg.detach(), gg.detach(), bg.detach(), rm1, rv1, EPS, 1.0, act, 0.01)
    var64 = x.double().var((0, 2, 3), unbiased=False)
    check("batchnorm running_var,momentum 1" + case, rv1, var64 * (n / (n - 1.0)), x.var((0, 2, 3), unbiased=True))
    assert ((rv1.cpu().double() / var64 - n / (n - 1.0)).abs() < 1e-3 / n).all()
    # accumulating into given dgamma / dbeta buffers
    _, mean, rstd = N.batchnorm_fwd(xg.detach(), gg.detach(), bg.detach(), None, None, EPS, 0.1, act, 0.01)
    pre_g, pre_b = torch.randn(shape[1], generator=gen(50)), torch.randn(shape[1], generator=gen(51))
    og, ob = pre_g.to(cuda), pre_b.to(cuda)
    dx, _, _ = N.batchnorm_bwd(dy.to(cuda), xg.detach(), gg.detach(), bg.detach(), mean, rstd, act, 0.01, out=(og, ob))
    assert torch.equal(bits(dx), bits(xg.grad))
    check("batchnorm_bwd dgamma,accumulate" + case, og, pre_g.double() + g64.grad, pre_g + g32.grad)
    check("batchnorm_bwd dbeta,accumulate" + case, ob, pre_b.double() + b64.grad, pre_b + b32.grad)


def test_batch_norm_layer_refuses_one_value_per_channel(cuda):
    from scda_amd import layers as L
    bn = L.BatchNorm2d(3).to(cuda).train()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    x = torch.randn(1, 3, 1, 1, device=cuda)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(x)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        torch.nn.BatchNorm2d(3).train()(x.cpu())
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
    assert torch.isfinite(bn.eval()(x)).all()           # eval mode normalises a single value with the running statistics
    assert torch.isfinite(bn.train()(torch.randn(2, 3, 1, 1, device=cuda))).all() and torch.isfinite(bn.running_var).all()


@pytest.mark.parametrize("act", [0, 1, 2])
def test_batch_norm_eval(cuda, act):
    from scda_amd import autograd_ops as A
    x, g, b, rm, rv, dy = bn_case((2, 3, 4, 5), 52)
    x64 = x.double().requires_grad_(); y64 = R.batch_norm_eval(x64, g, b, rm, rv, EPS, act, 0.01); y64.backward(dy.double())
    x32 = x.clone().requires_grad_(); y32 = ACT_FN[act](F.batch_norm(x32, rm, rv, g, b, False, 0.1, EPS)); y32.backward(dy)
    xg = x.to(cuda).requires_grad_()
    yg = A.BatchNormEvalFn.apply(xg, g.to(cuda), b.to(cuda), rm.to(cuda), rv.to(cuda), EPS, act, 0.01); yg.backward(dy.to(cuda))
    check(f"batchnorm_eval_fwd[act={act}]", yg, y64, y32)
    check(f"batchnorm_eval_bwd[act={act}]", xg.grad, x64.grad, x32.grad)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 1, 5), (2, 1, 3, 1), (1, 1, 3, 6)])
def test_upsample2x_thin_inputs(cuda, shape):
    from scda_amd import autograd_ops as A
    x = torch.randn(*shape, generator=gen(58)); dy = torch.randn(shape[0], shape[1], 2 * shape[2], 2 * shape[3], generator=gen(59))
    x64 = x.double().requires_grad_(); y64 = R.upsample2x(x64); y64.backward(dy.double())
    x32 = x.clone().requires_grad_(); y32 = F.interpolate(x32, scale_factor=2, mode="bilinear", align_corners=True); y32.backward(dy)
    xg = x.to(cuda).requires_grad_(); yg = A.Upsample2xFn.apply(xg); yg.backward(dy.to(cuda))
    check(f"upsample2x_fwd{shape}", yg, y64, y32)
    check(f"upsample2x_bwd{shape}", xg.grad, x64.grad, x32.grad)


# ------------------------------------------------------------------------- Adam
def adam_buffers(n, cuda, seed):
    p = torch.randn(n, generator=gen(seed))
    pg = torch.zeros((n + 3) // 4 * 4, device=cuda)[:n]; pg.copy_(p)
    return p, pg, torch.zeros_like(pg), torch.zeros_like(pg)


def test_adam_grid_cap_and_edges(cuda):
    from scda_amd import native as N
    n = 1027
    grads = [torch.randn(n, generator=gen(61 + i)) * 0.1 for i in range(3)]
    runs = {}
    for cap in (1, 0, 4096):            # one workgroup strides the whole bucket; the default; more workgroups than work
        p, pg, m, v = adam_buffers(n, cuda, 60)
        for i, g in enumerate(grads):
            N.adam_step(pg, g.to(cuda), m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-4, i + 1, max_blocks=cap)
        runs[cap] = (pg, m, v)
    for cap in (1, 4096):
        for got, want in zip(runs[cap], runs[0]):
            assert torch.equal(bits(got), bits(want)), cap
    lr, b1, b2, eps, wd = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8, 1e-4))       # the kernel's float arguments
    p64, m64, v64 = p.double(), torch.zeros(n).double(), torch.zeros(n).double()
    p32 = p.clone().requires_grad_()
    opt = torch.optim.Adam([p32], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    for i, g in enumerate(grads):
        p64, m64, v64 = R.adam_step(p64, g.double(), m64, v64, lr, b1, b2, eps, wd, i + 1)
        p32.grad = g.clone(); opt.step()
    check("adam[3 steps,n=1027] update", runs[0][0].cpu().double() - p.double(), p64 - p.double(), p32.detach().double() - p.double())
    # a late step from a warm state: the bias corrections are 1 - 0.9^1e5 = 1 and 1 - 0.999^1e5 = 1 - 3.5e-44
    g = grads[0]
    pg, m, v = runs[0]
    start = tuple(t.cpu().double() for t in (pg, m, v))
    p0 = pg.clone()
    N.adam_step(pg, g.to(cuda), m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 100000)
    want = R.adam_step(start[0], g.double(), start[1], start[2], lr, b1, b2, eps, wd, 100000)
    p32 = p0.cpu().clone()
    gr = g + 1e-4 * p32
    m32 = 0.9 * start[1].float() + (1 - 0.9) * gr; v32 = 0.999 * start[2].float() + (1 - 0.999) * gr * gr
    p32 = p32 - 1e-3 * m32 / (v32.sqrt() + 1e-8)
    check("adam[step=100000] update", pg.cpu().double() - start[0], want[0] - start[0], p32.double() - start[0])
    check("adam[step=100000] exp_avg", m, want[1], m32)
    check("adam[step=100000] exp_avg_sq", v, want[2], v32)
    # no decay, an all-zero gradient, a cold state: nothing moves (0 / (0 + eps))
    p, pg, m, v = adam_buffers(n, cuda, 64)
    N.adam_step(pg, torch.zeros(n, device=cuda), m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert torch.equal(bits(pg), bits(p)) and not m.any() and not v.any()


def test_adam_refuses_an_offset_view(cuda):
    from scda_amd import native as N
    n = 1027
    p = torch.randn(n, generator=gen(65))
    pv = offset_view(p, cuda)
    g = torch.randn(n, generator=gen(66)).to(cuda); m = torch.zeros(n, device=cuda); v = torch.zeros(n, device=cuda)
    with pytest.raises(N.ScdaNativeError, match="16-byte aligned"):
        N.adam_step(pv, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1)
    assert torch.equal(bits(pv), bits(p)) and not m.any() and not v.any()
