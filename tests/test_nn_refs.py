"""The fp64 restatements of tests/nn_refs.py against torch.nn.functional in double, at the shapes of tests/test_nn_ops_edges_gpu.py
(shrunk where a CPU would take long).  Hand-written gradients pass torch.autograd.gradcheck.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import nn_refs as R

TINY = 1e-12      # fp64 restatement vs torch's fp64: a few hundred ulp of slack for a different summation order


def gen(seed):
    return torch.Generator().manual_seed(seed)


def same(a, b, tol=TINY, equal_nan=False):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if equal_nan:
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        inf = float("inf")
        a, b = torch.nan_to_num(a, nan=0.0, posinf=inf, neginf=-inf), torch.nan_to_num(b, nan=0.0, posinf=inf, neginf=-inf)
    fin = torch.isfinite(b)
    assert torch.equal(a[~fin], b[~fin])
    scale = max(b[fin].abs().max().item(), 1e-20) if fin.any() else 1.0      # (all-zero expectations: absolute)
    err = (a[fin] - b[fin]).abs().max().item() / scale if fin.any() else 0.0
    assert err <= tol, err


EDGE = torch.tensor([100.0, -100.0, float("inf"), float("-inf"), -0.0, 0.0, 1e-30, -1e-30])


@pytest.mark.parametrize("mode,fn", [("relu", F.relu), ("leaky", lambda t: F.leaky_relu(t, 0.01)), ("tanh", torch.tanh),
                                     ("sigmoid", torch.sigmoid)])
@pytest.mark.parametrize("n", [1, 255, 257, 4101])
def test_activations(mode, fn, n):
    x = torch.cat([torch.randn(n, generator=gen(1)).double() * 3, EDGE.double()])
    xr = x.clone().requires_grad_()
    y = fn(xr)
    dy = torch.randn(y.shape, generator=gen(2)).double()
    y.backward(dy)
    same(R.act_fwd(x, mode), y, 1e-15)
    same(R.act_bwd(dy, y.detach(), mode), xr.grad, 1e-15)


def test_add_relu_axpby_dropout():
    a = torch.randn(257, generator=gen(3)).double(); b = torch.randn(257, generator=gen(4)).double()
    same(R.add_relu(a, b), F.relu(a + b), 0.0)
    same(R.axpby(a, b, 0.3, -1.7), 0.3 * a - 1.7 * b, 0.0)
    same(R.axpby(a, None, 0.3, 5.0), 0.3 * a, 0.0)
    keep = torch.rand(257, generator=gen(5)) < 0.5
    same(R.dropout_apply(a, keep, 2.0), a * keep.double() * 2.0, 0.0)


@pytest.mark.parametrize("hw", [(7, 9), (8, 12)])
def test_maxpools(hw):
    x = R.pool_input((2, 3) + hw, 6).double()
    y, idx = R.maxpool2x2(x)
    xr = x.clone().requires_grad_()
    yt = F.max_pool2d(xr, 2, 2)
    same(y, yt, 0.0, equal_nan=True)
    dy = torch.randn(y.shape, generator=gen(7)).double()
    yt.backward(dy)
    same(R.maxpool2x2_bwd(dy, idx, x.shape), xr.grad, 0.0)
    same(R.maxpool3x3s2(x), F.max_pool2d(x, 3, 2, 1), 0.0, equal_nan=True)


@pytest.mark.parametrize("shape", [(3, 5, 8, 8), (1, 2, 2, 2), (2, 3, 5, 9)])
def test_avg2x2s1(shape):
    x = torch.randn(*shape, generator=gen(8)).double()
    same(R.avg2x2s1(x), F.avg_pool2d(x, 2, 1))


@pytest.mark.parametrize("MN", [(1, 1), (7, 33), (9, 31), (513, 100)])
def test_colsum_rowmean(MN):
    x = torch.randn(*MN, generator=gen(9)).double()
    same(R.colsum(x), x.sum(0)); same(R.row_mean(x), x.mean(1))


@pytest.mark.parametrize("shape", [(1, 1, 2048), (2, 3, 2049), (1, 2500, 49), (4, 16, 1)])
def test_bias_grad_gap(shape):
    x = torch.randn(*shape, generator=gen(10)).double()
    same(R.bias_grad_nchw(x), x.sum((0, 2)))
    x4 = x.reshape(shape[0], shape[1], shape[2], 1)
    same(R.gap(x4), F.adaptive_avg_pool2d(x4, 1).flatten(1))


@pytest.mark.parametrize("Rr,C,scale,keep", [(1, 1, 3, 1), (1, 5, 3, 1), (1025, 2, 3, None), (77, 5, 3, None), (77, 5, 1e4, None),
                                            (77, 5, 3, 1)])
def test_cross_entropy_softmax_accuracy(Rr, C, scale, keep):
    x, t = R.ce_case(Rr, C, scale, keep)
    x = x.double()
    xa = x.clone().requires_grad_(); xb = x.clone().requires_grad_()
    la = R.cross_entropy(xa, t, -1); la.backward()
    lb = F.cross_entropy(xb, t, ignore_index=-1); lb.backward()
    same(la, lb); same(xa.grad, xb.grad)
    same(R.row_softmax(x), F.softmax(x, 1))
    v = t != -1
    same(R.accuracy(x, t, -1), (x[v].argmax(1) == t[v]).double().mean() * 100)


def test_cross_entropy_and_accuracy_all_ignored_and_ties():
    x = torch.randn(9, 4, generator=gen(14)).double()
    t = torch.full((9,), -1, dtype=torch.int64)
    assert torch.isnan(R.cross_entropy(x, t, -1)) and torch.isnan(F.cross_entropy(x, t, ignore_index=-1))
    assert torch.isnan(R.accuracy(x, t, -1)) and torch.isnan(torch.empty(0).mean())
    x = R.TIES.double()
    for t in (torch.tensor([0, 1, 0, 1]), torch.tensor([1, 2, 2, 1])):
        same(R.accuracy(x, t, -1), (x.argmax(1) == t).double().mean() * 100, 0.0)
    assert x.argmax(1).tolist() == [0, 1, 0, 1]


@pytest.mark.parametrize("with_mask", [True, False])
def test_smooth_l1(with_mask):
    n = 4099
    p = torch.randn(n, generator=gen(15)).double(); t = torch.randn(n, generator=gen(16)).double() * 0.5
    m = (torch.rand(n, generator=gen(17)) < 0.3).double() if with_mask else None
    pa = p.clone().requires_grad_(); pb = p.clone().requires_grad_()
    la = R.smooth_l1_sum(pa, m, t, 3.0, 0.25); la.backward()
    d = (pb * m if with_mask else pb) - t
    lb = F.smooth_l1_loss(d * 9.0, torch.zeros_like(d), reduction="sum", beta=1.0) / 9.0 * 0.25   # huber(9 d) / 9: the sigma form
    lb.backward()
    same(la, lb); same(pa.grad, pb.grad)
    # the stated convention at d = 0 and either side of 1 / sigma^2
    thr = 1.0 / 9.0
    q = torch.tensor([0.0, thr * (1 - 1e-9), thr, thr * (1 + 1e-9), -thr, -thr * (1 - 1e-9)], dtype=torch.float64).requires_grad_()
    R.smooth_l1_sum(q, None, torch.zeros(6), 3.0).backward()
    assert R.smooth_l1_branch(q, None, torch.zeros(6), 3.0).tolist() == [True, True, False, False, False, True]
    assert q.grad[0].item() == 0.0 and q.grad[2].item() == 1.0 and q.grad[4].item() == -1.0
    # gradcheck away from the kinks
    pg = (torch.randn(12, generator=gen(18)).double() * 0.4).requires_grad_()
    tg = torch.zeros(12).double()
    assert ((pg.detach().abs() - thr).abs() > 1e-3).all() and (pg.detach().abs() > 1e-3).all()
    mg = torch.rand(12, generator=gen(19)).double() + 0.5
    assert torch.autograd.gradcheck(lambda v: R.smooth_l1_sum(v, mg, tg, 3.0, 0.7), (pg,))


def test_bce():
    p = torch.rand(1024, generator=gen(23)).clamp(1e-6, 1 - 1e-6).double(); p[0] = 0.0; p[1] = 1.0
    t = torch.rand(1024, generator=gen(24)).double()
    pa = p.clone().requires_grad_(); pb = p.clone().requires_grad_()
    la = R.bce(pa, t); la.backward()
    lb = F.binary_cross_entropy(pb, t); lb.backward()
    same(la, lb); same(pa.grad, pb.grad, 1e-8)      # torch holds the clamp as a float: 1e-12f = 1e-12 (1 - 4e-9)
    same(pa.grad[:2], torch.stack([-t[0], 1.0 - t[1]]) / 1e-12 / 1024, 1e-15)
    pg = (torch.rand(10, generator=gen(25)).double() * 0.8 + 0.1).requires_grad_()
    assert torch.autograd.gradcheck(lambda v: R.bce(v, t[:10]), (pg,))


@pytest.mark.parametrize("C,n", [(1, 1), (5, 1023), (1, 1025), (5, 1)])
def test_adversarial_loss(C, n):
    groups_a, groups_b, lb = [], [], 0.0
    for k in range(2):
        x = torch.randn(C, n, generator=gen(26 + k)).double() * 3
        t = (torch.rand(1 if k == 0 else C, n, generator=gen(28 + k)) < 0.5).double()
        x[0, 0] = 100.0; t[0, 0] = 0.0                  # both logs at their clamp
        if n > 1:
            x[0, 1] = -100.0; x[-1, -1] = -100.0; t[0, 1] = 1.0
        w = torch.rand(C, generator=gen(30 + k)).double(); w[0] = 0.0
        xa = x.clone().requires_grad_(); xb = x.clone().requires_grad_()
        groups_a.append((xa, t, w if k == 0 else None)); groups_b.append(xb)
        for c in range(C):
            lb = lb + (w[c] if k == 0 else 1.0) * F.binary_cross_entropy(torch.sigmoid(xb[c]), t[c if k else 0])
    la = R.adversarial_loss(groups_a, 0.37); la.backward()
    (lb * 0.37).backward()
    same(la, lb * 0.37)
    for (xa, _, _), xb in zip(groups_a, groups_b):
        same(xa.grad, xb.grad, 1e-8)                    # torch's float clamp constant again


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (31, 33), (25, 41)])
def test_instance_norm(act, hw):
    x = (torch.randn(2, 3, *hw, generator=gen(32)) * 2 + 0.5).double()
    x[0, 1] = 2.5                                       # a constant plane
    x[1, 0] = 1e3 + 1e-2 * torch.randn(*hw, generator=gen(33)).double()
    f = [lambda v: v, F.relu, lambda v: F.leaky_relu(v, 0.01)][act]
    xa = x.clone().requires_grad_(); xb = x.clone().requires_grad_()
    ya, mean, rstd = R.instance_norm(xa, 1e-5, act, 0.01)
    dy = torch.randn(ya.shape, generator=gen(34)).double()
    ya.backward(dy)
    if hw != (1, 1):                                    # torch refuses one value per plane; there y = 0 and dx = 0 by the formula
        yb = f(F.instance_norm(xb, eps=1e-5))
        yb.backward(dy)
        same(ya, yb, 1e-9); same(xa.grad, xb.grad, 1e-7)    # 1e3 +- 1e-2: the variance's own conditioning, 1e10 x 1e-16
    else:
        assert not ya.any() and not xa.grad.any()
    assert (ya[0, 1] == 0).all() and torch.isfinite(xa.grad).all()
    same(rstd[1:2], torch.tensor([1e-5], dtype=torch.float64).rsqrt(), 1e-15)
    same(mean, x.mean((2, 3)).reshape(-1), 1e-15)


def test_instnorm_drop_add():
    x = torch.randn(2, 2, 5, 7, generator=gen(35)).double(); r = torch.randn(2, 2, 5, 7, generator=gen(36)).double()
    keep = torch.rand(2, 2, 5, 7, generator=gen(37)) < 0.5
    y, _, _ = R.instnorm_drop_add(x, r, keep, 1e-5, 0.5)
    same(y, r + F.instance_norm(x, eps=1e-5) * keep.double() * 2.0)


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (4, 10, 8, 8), (1, 4, 1, 4)])
def test_batch_norm_train(shape, act):
    C = shape[1]
    x = torch.randn(*shape, generator=gen(38)).double() * 2 + 0.3
    g = torch.rand(C, generator=gen(39)).double() + 0.5; b = torch.randn(C, generator=gen(40)).double()
    rm0 = torch.randn(C, generator=gen(41)).double(); rv0 = torch.rand(C, generator=gen(42)).double() + 0.5
    xa, ga, ba = (v.clone().requires_grad_() for v in (x, g, b))
    xb, gb, bb = (v.clone().requires_grad_() for v in (x, g, b))
    ya, rm, rv, mean, rstd = R.batch_norm_train(xa, ga, ba, rm0, rv0, 1e-5, 0.1, act, 0.01)
    rmt, rvt = rm0.clone(), rv0.clone()
    yb = F.batch_norm(xb, rmt, rvt, gb, bb, True, 0.1, 1e-5)
    if act == 2:
        yb = F.leaky_relu(yb, 0.01)
    dy = torch.randn(ya.shape, generator=gen(43)).double()
    ya.backward(dy); yb.backward(dy)
    same(ya, yb, 1e-10); same(xa.grad, xb.grad, 1e-9); same(ga.grad, gb.grad, 1e-10); same(ba.grad, bb.grad, 1e-10)
    same(rm, rmt); same(rv, rvt)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_batch_norm_eval(act):
    x = torch.randn(2, 3, 4, 5, generator=gen(44)).double()
    g = torch.rand(3, generator=gen(45)).double() + 0.5; b = torch.randn(3, generator=gen(46)).double()
    rm = torch.randn(3, generator=gen(47)).double(); rv = torch.rand(3, generator=gen(48)).double() + 0.5
    f = [lambda v: v, F.relu, lambda v: F.leaky_relu(v, 0.01)][act]
    xa = x.clone().requires_grad_(); xb = x.clone().requires_grad_()
    ya = R.batch_norm_eval(xa, g, b, rm, rv, 1e-5, act, 0.01); yb = f(F.batch_norm(xb, rm, rv, g, b, False, 0.1, 1e-5))
    dy = torch.randn(ya.shape, generator=gen(49)).double()
    ya.backward(dy); yb.backward(dy)
    same(ya, yb); same(xa.grad, xb.grad)
    xg = x.clone().requires_grad_()
    assert (R.batch_norm_eval(x, g, b, rm, rv, 1e-5).abs() > 1e-3).all()          # away from the activation's kink
    assert torch.autograd.gradcheck(lambda v: R.batch_norm_eval(v, g, b, rm, rv, 1e-5, act, 0.01), (xg,))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 1, 5), (2, 1, 3, 1), (1, 1, 3, 6)])
def test_upsample2x(shape):
    x = torch.randn(*shape, generator=gen(50)).double()
    xa = x.clone().requires_grad_(); xb = x.clone().requires_grad_()
    ya = R.upsample2x(xa); yb = F.interpolate(xb, scale_factor=2, mode="bilinear", align_corners=True)
    dy = torch.randn(ya.shape, generator=gen(51)).double()
    ya.backward(dy); yb.backward(dy)
    same(ya, yb); same(xa.grad, xb.grad)


def test_adam():
    n = 1027
    p = torch.randn(n, generator=gen(52)).double()
    pr = p.clone().requires_grad_()
    opt = torch.optim.Adam([pr], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    m = torch.zeros(n).double(); v = torch.zeros(n).double()
    for i in range(3):
        g = torch.randn(n, generator=gen(53 + i)).double() * 0.1
        pr.grad = g.clone(); opt.step()
        p, m, v = R.adam_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-4, i + 1)
    same(p, pr, 1e-14)
    # zero gradient, no decay: nothing moves; a late step: the bias corrections are ~1
    p0 = torch.randn(8, generator=gen(56)).double()
    p1, m1, v1 = R.adam_step(p0, torch.zeros(8).double(), torch.zeros(8).double(), torch.zeros(8).double(), 1e-3, 0.9, 0.999, 1e-8, 0.0, 100000)
    assert torch.equal(p1, p0) and not m1.any() and not v1.any()
