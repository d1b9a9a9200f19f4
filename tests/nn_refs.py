"""fp64 restatements, on the CPU, of the layer and loss operations of scda_amd/csrc/nn_ops.hip.

Every forward is written out from its formula in torch double; gradients come from torch autograd in double, except where the
kernels document a convention of their own -- those are written out as torch.autograd.Function with the stated formula:
  * BCE:        d/dp = (p - t) / max(p (1 - p), 1e-12) / n     (torch's clamp)
  * smooth-L1:  sign(0) = 0, quadratic branch for |d| < 1 / sigma^2 (strictly)
  * eval-mode batch norm: statistics and affine parameters are constants, dx = dy * act'(y) * gamma * rstd
Nothing here is shared with scda_amd or oracle/.  tests/test_nn_refs.py checks this file against torch.nn.functional."""
import torch


def f64(t):
    return t.detach().cpu().double()


# ------------------------------------------------------------------ element-wise
def act_fwd(x, mode, slope=0.01):
    """mode: 'relu' | 'leaky' | 'tanh' | 'sigmoid'"""
    x = f64(x)
    if mode == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    if mode == "leaky":
        return torch.where(x > 0, x, x * slope)
    if mode == "tanh":
        return 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)
    if mode == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    raise ValueError(mode)


def act_bwd(dy, y, mode, slope=0.01):
    """gradient w.r.t. the activation's input, from its OUTPUT y"""
    dy, y = f64(dy), f64(y)
    if mode == "relu":
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if mode == "leaky":
        return torch.where(y > 0, dy, dy * slope)
    if mode == "tanh":
        return dy * (1.0 - y * y)
    if mode == "sigmoid":
        return dy * y * (1.0 - y)
    raise ValueError(mode)


def add_relu(a, b):
    s = f64(a) + f64(b)
    return torch.where(s > 0, s, torch.zeros_like(s))


def axpby(a, b, alpha, beta):
    return alpha * f64(a) + (beta * f64(b) if b is not None else 0.0)


def dropout_apply(x, keep, scale):
    x = f64(x)
    return torch.where(keep.cpu().bool(), x * scale, torch.zeros_like(x))


# ------------------------------------------------------------------------ pools
def _take(cand, m):
    return (cand > m) | torch.isnan(cand)        # a NaN always wins, the last one stays


def maxpool2x2(x):
    """-> (y, idx): idx = dy * 2 + dx of the winner; ties: the first; floor mode"""
    x = f64(x)
    OH, OW = x.shape[-2] // 2, x.shape[-1] // 2
    m = x[..., 0:2 * OH:2, 0:2 * OW:2].clone()
    k = torch.zeros(m.shape, dtype=torch.int64)
    for j, (dy, dx) in enumerate(((0, 1), (1, 0), (1, 1)), start=1):
        c = x[..., dy:2 * OH:2, dx:2 * OW:2]
        t = _take(c, m)
        m = torch.where(t, c, m)
        k = torch.where(t, torch.full_like(k, j), k)
    return m, k


def maxpool2x2_bwd(dy, idx, x_shape):
    dy = f64(dy)
    dx = torch.zeros(x_shape, dtype=torch.float64)
    OH, OW = dy.shape[-2:]
    for j, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[..., a:2 * OH:2, b:2 * OW:2] = torch.where(idx == j, dy, torch.zeros_like(dy))
    return dx


def maxpool3x3s2(x):
    """kernel 3, stride 2, padding 1 with -inf padding"""
    x = f64(x)
    H, W = x.shape[-2:]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full(x.shape[:-2] + (2 * OH + 1, 2 * OW + 1), float("-inf"), dtype=torch.float64)
    xp[..., 1:H + 1, 1:W + 1] = x
    m = torch.full(x.shape[:-2] + (OH, OW), float("-inf"), dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            c = xp[..., dy:dy + 2 * OH:2, dx:dx + 2 * OW:2]
            m = torch.where(_take(c, m), c, m)
    return m


def avg2x2s1(x):
    x = x.double()
    return (x[..., :-1, :-1] + x[..., :-1, 1:] + x[..., 1:, :-1] + x[..., 1:, 1:]) * 0.25


def gap(x):
    x = x.double()
    return x.reshape(x.shape[0], x.shape[1], -1).sum(-1) / (x.shape[2] * x.shape[3])


# -------------------------------------------------------------------- reductions
def colsum(dy):
    return f64(dy).sum(0)


def bias_grad_nchw(dy):
    dy = f64(dy)
    return dy.reshape(dy.shape[0], dy.shape[1], -1).sum((0, 2))


def row_mean(x):
    return f64(x).sum(1) / x.shape[1]


# ------------------------------------------------------------------------ losses
def log_softmax_rows(x):
    x = x.double()
    z = x - x.max(1, keepdim=True).values
    return z - torch.log(torch.exp(z).sum(1, keepdim=True))


def cross_entropy(logits, targets, ignore_index):
    """mean over the rows whose target is not ignore_index (0 / 0 = NaN when there is none); differentiable w.r.t. logits"""
    ls = log_softmax_rows(logits)
    valid = targets != ignore_index
    pick = ls.gather(1, torch.where(valid, targets, torch.zeros_like(targets)).reshape(-1, 1)).reshape(-1)
    return -(pick * valid.double()).sum() / valid.double().sum()


def row_softmax(x):
    return torch.exp(log_softmax_rows(f64(x)))


def accuracy(logits, targets, ignore_index):
    """percent of the rows with a target whose FIRST maximum is the target (0 / 0 = NaN when there is none)"""
    x = f64(logits)
    valid = targets != ignore_index
    best = torch.zeros(x.shape[0], dtype=torch.int64)
    bv = x[:, 0].clone()
    for c in range(1, x.shape[1]):
        t = x[:, c] > bv
        bv = torch.where(t, x[:, c], bv)
        best = torch.where(t, torch.full_like(best, c), best)
    ok = ((best == targets) & valid).double().sum()
    return ok * (100.0 / valid.double().sum())


class _SmoothL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, mask, target, sigma2):
        d = pred * mask - target
        a = d.abs()
        quad = a < 1.0 / sigma2
        ctx.save_for_backward(d, mask, quad)
        ctx.sigma2 = sigma2
        return torch.where(quad, d * d * sigma2 * 0.5, a - 0.5 / sigma2).sum()

    @staticmethod
    def backward(ctx, g):
        d, mask, quad = ctx.saved_tensors
        sign = (d > 0).double() - (d < 0).double()          # 0 at d = 0
        return torch.where(quad, d * ctx.sigma2, sign) * mask * g, None, None, None


def smooth_l1_sum(pred, mask, target, sigma, scale=1.0):
    """scale * sum smooth_l1(pred * mask - target); pred double, differentiable"""
    m = torch.ones_like(pred) if mask is None else f64(mask)
    return _SmoothL1.apply(pred, m, f64(target), float(sigma) * float(sigma)) * scale


def smooth_l1_branch(pred, mask, target, sigma):
    """True where the quadratic branch is taken"""
    d = f64(pred) * (1.0 if mask is None else f64(mask)) - f64(target)
    return d.abs() < 1.0 / (float(sigma) * float(sigma))


class _BCE(torch.autograd.Function):
    """element-wise -(t log p + (1 - t) log(1 - p)), logs clamped at -100; gradient with torch's clamp of the denominator"""

    @staticmethod
    def forward(ctx, p, t):
        ctx.save_for_backward(p, t)
        lp = torch.log(p).clamp(min=-100.0)
        l1p = torch.log1p(-p).clamp(min=-100.0)
        return -(t * lp + (1.0 - t) * l1p)

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        return g * (p - t) / ((1.0 - p) * p).clamp(min=1e-12), None


def bce(p, t):
    """mean binary cross entropy of probabilities; p double, differentiable"""
    return _BCE.apply(p, f64(t)).sum() / p.numel()


def adversarial_loss(groups, scale):
    """scale * sum over groups (logits [C,n] double, labels [1,n] | [C,n], weights [C] | None) of sum_c w[c] * mean_i BCE(sigmoid(x), t)"""
    total = 0.0
    for x, t, w in groups:
        p = 1.0 / (1.0 + torch.exp(-x))
        rows = _BCE.apply(p, f64(t).expand_as(x).contiguous()).sum(1) / x.shape[1]
        total = total + (rows * (f64(w) if w is not None else 1.0)).sum()
    return total * scale


# ------------------------------------------------------------------------- norms
def _act(y, act, slope):
    """act: 0 none, 1 relu, 2 leaky"""
    if act == 1:
        return torch.where(y > 0, y, torch.zeros_like(y))
    if act == 2:
        return torch.where(y > 0, y, y * slope)
    return y


def instance_norm(x, eps, act=0, slope=0.01):
    """-> (y, mean [B*C], rstd [B*C]); x double, y differentiable"""
    B, C, H, W = x.shape
    p = x.reshape(B * C, H * W)
    mean = p.sum(1, keepdim=True) / (H * W)
    var = ((p - mean) ** 2).sum(1, keepdim=True) / (H * W)
    rstd = 1.0 / torch.sqrt(var + eps)
    return _act(((p - mean) * rstd).reshape(x.shape), act, slope), mean.reshape(-1), rstd.reshape(-1)


def instnorm_drop_add(x, residual, keep, eps, p):
    """residual + dropout(instance_norm(x)) with the keep decisions given"""
    y, mean, rstd = instance_norm(x, eps)
    return residual + torch.where(keep.cpu().bool(), y * (1.0 / (1.0 - p)), torch.zeros_like(y)), mean, rstd


def batch_norm_train(x, gamma, beta, run_mean, run_var, eps, momentum, act=0, slope=0.01):
    """-> (y, new running mean, new running var (unbiased estimate), mean, rstd); x / gamma / beta double, y differentiable"""
    B, C, H, W = x.shape
    n = B * H * W
    mean = x.sum((0, 2, 3)) / n
    var = ((x - mean.reshape(1, C, 1, 1)) ** 2).sum((0, 2, 3)) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean.reshape(1, C, 1, 1)) * rstd.reshape(1, C, 1, 1) * gamma.reshape(1, C, 1, 1) + beta.reshape(1, C, 1, 1)
    new_mean = (1.0 - momentum) * f64(run_mean) + momentum * mean.detach()
    new_var = (1.0 - momentum) * f64(run_var) + momentum * var.detach() * (n / (n - 1.0))
    return _act(y, act, slope), new_mean, new_var, mean.detach(), rstd.detach()


class _BNEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, mean, var, eps, act, slope):
        C = x.shape[1]
        rstd = 1.0 / torch.sqrt(var + eps)
        y = (x - mean.reshape(1, C, 1, 1)) * (rstd * gamma).reshape(1, C, 1, 1) + beta.reshape(1, C, 1, 1)
        ctx.save_for_backward(y, rstd * gamma)
        ctx.cfg = (act, slope)
        return _act(y, act, slope)

    @staticmethod
    def backward(ctx, dy):
        y, k = ctx.saved_tensors
        act, slope = ctx.cfg
        g = dy
        if act == 1:
            g = torch.where(y > 0, dy, torch.zeros_like(dy))
        elif act == 2:
            g = torch.where(y > 0, dy, dy * slope)
        return g * k.reshape(1, -1, 1, 1), None, None, None, None, None, None, None


def batch_norm_eval(x, gamma, beta, mean, var, eps, act=0, slope=0.01):
    return _BNEval.apply(x, f64(gamma), f64(beta), f64(mean), f64(var), eps, act, slope)


# ---------------------------------------------------------------------- upsample
def _up_matrix(n_in):
    """[2 n_in, n_in] bilinear weights, align_corners=True"""
    n_out = 2 * n_in
    w = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        src = o * (n_in - 1) / (n_out - 1)
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        f = src - i0
        w[o, i0] += 1.0 - f
        w[o, i1] += f
    return w


def upsample2x(x):
    """x double [B,C,H,W] -> [B,C,2H,2W]; differentiable"""
    return _up_matrix(x.shape[2]) @ x @ _up_matrix(x.shape[3]).t()


# -------------------------------------------------------------------------- Adam
def adam_step(p, g, m, v, lr, b1, b2, eps, wd, step):
    """torch.optim.Adam with L2-coupled decay; all double; -> (p, m, v)"""
    g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return p - (lr / bc1) * m / (torch.sqrt(v) / (bc2 ** 0.5) + eps), m, v


# ------------------------------------------------- inputs the two test files share
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def pool_input(shape, seed, edges=True):
    """fp32 ReLU output whose 2x2 windows are all-zero about a third of the time (P(0) = 0.76 per element); edges: NaN and -inf planted"""
    x = torch.relu(torch.randn(*shape, generator=_gen(seed)) - 0.7)
    x[0, 0, :4, :4] = 0.0
    if edges:
        x[0, 1, 0, 0] = float("nan"); x[0, 1, 2, 3] = float("nan"); x[0, 1, 3, 3] = float("nan")   # one alone, two in one window
        x[1, 0] = float("-inf"); x[1, 0, 1, 1] = 0.5                                                # windows of -inf only
        x[1, 1, 4:6, 2:4] = float("-inf")
    return x


def ce_case(rows, classes, scale, keep_rows, seed=11):
    """fp32 logits * scale and targets; keep_rows: None = about 40 % of the rows keep a target, else the first keep_rows do (rest -1)"""
    x = torch.randn(rows, classes, generator=_gen(seed)) * scale
    t = torch.randint(0, classes, (rows,), generator=_gen(seed + 1))
    if keep_rows is None:
        t[torch.rand(rows, generator=_gen(seed + 2)) < 0.6] = -1
        t[0] = 0
    else:
        t[keep_rows:] = -1
    return x, t


TIES = torch.tensor([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0], [0.0, 1.0, 0.5]])      # first maxima: 0, 1, 0, 1
