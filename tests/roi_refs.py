"""Plain references of the RoI operators, focal losses and overlap matrices of scda_amd/csrc/detection_ops.hip: no GPU, no C.
tests/test_roi_refs.py pins every one of them against the C oracle (oracle/scda_oracle.c); tests/test_roi_edges_gpu.py compares
the HIP kernels with them.

  roi_pool_fwd                  the fp32 restatement of tests/np_restate.py (values and argmax, bit for bit)
  roi_pool_bwd_reference_rule   roi_pooling_kernel.cu:128-203 as a scatter: fp32 sums in (roi, ph, pw) order over argmax hits, with the
                                reference's `in_roi` gate and its phstart .. pwend ranges
  roi_pool_bwd_pure_scatter     the same WITHOUT the gate and the ranges (what an argmax-driven scatter computes if it forgets them)
  roi_align                     roi_align_kernel.cu: fp32 sample geometry exactly as the kernel holds it, interpolation in fp64
  focal_sigmoid / focal_softmax the reference's formulas in float64 on the fp32 inputs
  iou_overlaps / bbox_overlaps  fp32 numpy, one rounding per operator"""
import numpy as np

import np_restate as npr

f32 = np.float32
f64 = np.float64
FLT_MIN = float(np.finfo(f32).tiny)

roi_pool_fwd = npr.roi_pool


# ---------------------------------------------------------------- RoI max pooling, backward
def _rects(rois, scale):
    v = (rois[:, 1:5].astype(f32) * f32(scale)).astype(f32)
    return npr.round_half_away(v)          # [R, 4] = sw, sh, ew, eh


def _pool_entries(arg, rois, feat_shape, PH, PW, scale, gated):
    """flat positions (in (roi, c, ph, pw) order) of the outputs whose argmax receives their gradient"""
    B, C, H, W = feat_shape
    R = arg.shape[0]
    a = arg.reshape(-1).astype(np.int64)
    keep = a >= 0
    if not gated or R == 0:
        return np.nonzero(keep)[0]
    i = np.arange(a.size)
    r, ph, pw = i // (C * PH * PW), (i // PW) % PH, i % PW
    rc = _rects(rois, scale)
    sw, sh, ew, eh = (rc[r, k] for k in range(4))
    w, h = a % W, (a // W) % H
    keep &= (w >= sw) & (w <= ew) & (h >= sh) & (h <= eh)                      # in_roi, :161-166
    bin_h = (np.maximum(eh - sh + 1, 1).astype(f32) / f32(PH)).astype(f32)      # :176-180
    bin_w = (np.maximum(ew - sw + 1, 1).astype(f32) / f32(PW)).astype(f32)
    with np.errstate(all="ignore"):
        phs = np.floor(((h - sh).astype(f32) / bin_h).astype(f32)); phe = np.ceil(((h - sh + 1).astype(f32) / bin_h).astype(f32))
        pws = np.floor(((w - sw).astype(f32) / bin_w).astype(f32)); pwe = np.ceil(((w - sw + 1).astype(f32) / bin_w).astype(f32))
    phs = np.clip(phs, 0, PH); phe = np.clip(phe, 0, PH); pws = np.clip(pws, 0, PW); pwe = np.clip(pwe, 0, PW)   # :187-190
    keep &= (ph >= phs) & (ph < phe) & (pw >= pws) & (pw < pwe)
    return np.nonzero(keep)[0]


def _ordered_scatter(top, arg, idx, feat_shape):
    g = np.zeros(int(np.prod(feat_shape)), f32)
    # ufunc.at is unbuffered and walks its index list front to back: every pixel's contributors are added one by one, in fp32, in
    # (roi, ph, pw) order (a pixel belongs to one channel).  tests/test_roi_refs.py checks this against an explicit loop.
    np.add.at(g, arg.reshape(-1)[idx].astype(np.int64), top.reshape(-1).astype(f32)[idx])
    return g.reshape(feat_shape)


def roi_pool_bwd_reference_rule(top, arg, rois, feat_shape, PH, PW, scale):
    return _ordered_scatter(top, arg, _pool_entries(arg, rois, feat_shape, PH, PW, scale, True), feat_shape)


def roi_pool_bwd_pure_scatter(top, arg, feat_shape):
    return _ordered_scatter(top, arg, _pool_entries(arg, None, feat_shape, arg.shape[2], arg.shape[3], 0.0, False), feat_shape)


# ---------------------------------------------------------------- RoIAlign
def roi_align(feat, rois, AH, AW, scale, top=None, stats=False):
    """A THIRD, independent statement of extensions/_roi_align/src/roi_align_kernel.cu:15-70 (forward) and :94-143 (backward), written
    from the kernel text by flat-index arithmetic only -- it shares no helper with oracle/scda_oracle.c or tests/np_restate.py.  Sample
    geometry in float32 exactly as the kernel's float variables hold it (the `1.` literals make the divisions double, the results are
    stored to float), interpolation in float64.  -> out [R, C, AH, AW] (float64), and with `top` the gradient [B, C, H, W].
    stats=True (with `top`): -> (out, grad, k, S, weights): per gradient pixel the number k of non-zero contributions and
    S = sum |contribution| (float64), and the bilinear weights of all contributions (channel 0's; they do not depend on the channel)."""
    B, C, H, W = feat.shape
    R = rois.shape[0]
    r = rois.astype(f32)
    sc = f32(scale)
    with np.errstate(invalid="ignore"):
        x1, y1, x2, y2 = (r[:, 1] * sc).astype(f32), (r[:, 2] * sc).astype(f32), (r[:, 3] * sc).astype(f32), (r[:, 4] * sc).astype(f32)
        rw = np.fmax((x2 - x1).astype(f64) + 1.0, 0.0).astype(f32)          # fmaxf(roi_end_w - roi_start_w + 1., 0.)
        rh = np.fmax((y2 - y1).astype(f64) + 1.0, 0.0).astype(f32)
        bh = (rh.astype(f64) / (AH - 1.0)).astype(f32)                          # roi_height / (aligned_height - 1.)
        bw = (rw.astype(f64) / (AW - 1.0)).astype(f32)
        ph = np.arange(AH, dtype=f32)[None, :]
        pw = np.arange(AW, dtype=f32)[None, :]
        h = (ph * bh[:, None] + y1[:, None]).astype(f32)                               # [R, AH]   (float)(ph) * bin_size_h + roi_start_h
        w = (pw * bw[:, None] + x1[:, None]).astype(f32)                               # [R, AW]
        hs = np.fmin(np.floor(h), f32(H - 2)).astype(np.int64)                         # fminf(floor(h), height - 2): a NaN gives height - 2
        ws = np.fmin(np.floor(w), f32(W - 2)).astype(np.int64)
        inside = ~((h < 0) | (h >= H))[:, :, None] & ~((w < 0) | (w >= W))[:, None, :] # [R, AH, AW]
        hr = (h - hs.astype(f32)).astype(f32).astype(f64)[:, :, None]           # h_ratio (float), used in double arithmetic
        wr = (w - ws.astype(f32)).astype(f32).astype(f64)[:, None, :]
    img = r[:, 0].astype(np.int64)
    base = img[:, None, None] * (C * H * W) + np.where(inside, hs[:, :, None] * W + ws[:, None, :], 0)   # channel 0's up-left corner
    flat = feat.astype(f64).reshape(-1)
    coef = [(1.0 - hr) * (1.0 - wr), (1.0 - hr) * wr, hr * (1.0 - wr), hr * wr]
    offs = [0, 1, W, W + 1]
    chan = (np.arange(C, dtype=np.int64) * (H * W))[None, :, None, None]
    idx0 = base[:, None, :, :] + chan                                               # [R, C, AH, AW]
    out = np.zeros((R, C, AH, AW))
    with np.errstate(invalid="ignore"):
        for cf, o in zip(coef, offs):
            out += flat[idx0 + o] * cf[:, None, :, :]
    out = np.where(inside[:, None, :, :], out, 0.0)
    if top is None:
        return out
    grad = np.zeros(B * C * H * W)
    k = np.zeros(B * C * H * W, np.int64)
    S = np.zeros(B * C * H * W)
    t = top.astype(f64) * inside[:, None, :, :]
    for cf, o in zip(coef, offs):
        contrib = (t * cf[:, None, :, :]).reshape(-1)
        np.add.at(grad, (idx0 + o).reshape(-1), contrib)
        if stats:
            np.add.at(k, (idx0 + o).reshape(-1), (contrib != 0).astype(np.int64))
            np.add.at(S, (idx0 + o).reshape(-1), np.abs(contrib))
    if not stats:
        return out, grad.reshape(B, C, H, W)
    weights = np.concatenate([cf[inside] for cf in coef])
    return out, grad.reshape(B, C, H, W), k.reshape(B, C, H, W), S.reshape(B, C, H, W), weights


# ---------------------------------------------------------------- focal losses (float64 on the fp32 inputs)
def _focal_z(weight_pos, alpha):
    Np = max(float(f32(weight_pos)), 1.0)
    a = float(f32(alpha))
    return (1.0 - a) / Np, a / Np          # zn, zp


def _sigmoid_terms(x, t, nc):
    x = x.astype(f64).reshape(-1, nc)
    d = np.arange(nc)[None, :]
    t = t.astype(np.int64)[:, None]
    c1 = (t == d + 1).astype(f64)
    c2 = ((t != -1) & (t != d + 1)).astype(f64)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        ge = (x >= 0).astype(f64)
        log1mp = -x * ge - np.log(1.0 + np.exp(x - 2.0 * x * ge))       # log(1 - p), the reference's stable form
    logp = np.log(np.maximum(p, FLT_MIN))
    return x, c1, c2, p, logp, log1mp


def focal_sigmoid_fwd(x, t, weight_pos, gamma, alpha, nc):
    """focal_loss_sigmoid_kernel.cu:12-47 -> [rows, nc] float64"""
    shape = x.shape
    x, c1, c2, p, logp, log1mp = _sigmoid_terms(x, t, nc)
    zn, zp = _focal_z(weight_pos, alpha)
    g = float(f32(gamma))
    return (-c1 * (1.0 - p) ** g * logp * zp - c2 * p ** g * log1mp * zn).reshape(shape)


def focal_sigmoid_bwd(x, t, weight_pos, gamma, alpha, nc):
    """focal_loss_sigmoid_kernel.cu:49-81"""
    shape = x.shape
    x, c1, c2, p, logp, log1mp = _sigmoid_terms(x, t, nc)
    zn, zp = _focal_z(weight_pos, alpha)
    g = float(f32(gamma))
    term1 = (1.0 - p) ** g * (1.0 - p - p * g * logp)
    term2 = p ** g * (log1mp * (1.0 - p) * g - p)
    return (-c1 * zp * term1 - c2 * zn * term2).reshape(shape)


def _softmax_z(t, weight_pos, alpha):
    zn, zp = _focal_z(weight_pos, alpha)
    return (t == 0) * zn + (t >= 1) * zp


def focal_softmax_fwd(x, t, weight_pos, gamma, alpha, nc):
    """SpatialSoftmaxKernel + SoftmaxFocalLossKernel (focal_loss_softmax_kernel.cu:12-57) -> (losses [rows], P [rows, nc]) float64"""
    x = x.astype(f64).reshape(-1, nc)
    t = t.astype(np.int64)
    e = np.exp(x - x.max(1, keepdims=True))
    P = e / e.sum(1, keepdims=True)
    pl = P[np.arange(len(t)), np.maximum(t, 0)]
    g = float(f32(gamma))
    l = -((1.0 - pl) ** g * np.log(np.maximum(pl, FLT_MIN))) * _softmax_z(t, weight_pos, alpha)
    return np.where(t >= 0, l, 0.0), P


def focal_softmax_bwd(P, t, weight_pos, gamma, alpha, nc):
    """GradientWeightKernel + GradientKernel (:59-100) on GIVEN probabilities P (the kernel's input) -> [rows, nc] float64.
    The weight's second term gamma (1 - p)^(gamma - 1) p log p is 0 at p = 1 for every gamma >= 0 (log p ~ -(1 - p)); evaluated
    literally it is 0 * inf for gamma < 1.  The limit is what is stated here."""
    P = P.astype(f64).reshape(-1, nc)
    t = t.astype(np.int64)
    p = P[np.arange(len(t)), np.maximum(t, 0)]
    g = float(f32(gamma))
    logp = np.log(np.maximum(p, FLT_MIN))
    with np.errstate(all="ignore"):
        second = np.where(logp == 0.0, 0.0, g * (1.0 - p) ** (g - 1.0) * p * logp)
        b = (-(1.0 - p) ** g + second) * _softmax_z(t, weight_pos, alpha)
    b = np.where(t >= 0, b, 0.0)
    onehot = (np.arange(nc)[None, :] == t[:, None]).astype(f64)
    return (t >= 0)[:, None] * b[:, None] * (onehot - P)


# ---------------------------------------------------------------- overlap matrices (fp32, one rounding per operator)
def iou_overlaps(b1, b2):
    """iou_overlap_kernel.cu:33-65: no +1, union clamped to >= 1.  Boxes may carry extra columns (size_bbox 5)."""
    p, q = b1.astype(f32)[:, None, :], b2.astype(f32)[None, :, :]
    with np.errstate(all="ignore"):
        a1 = ((p[..., 2] - p[..., 0]).astype(f32) * (p[..., 3] - p[..., 1]).astype(f32)).astype(f32)
        a2 = ((q[..., 2] - q[..., 0]).astype(f32) * (q[..., 3] - q[..., 1]).astype(f32)).astype(f32)
        width = np.maximum((np.minimum(p[..., 2], q[..., 2]) - np.maximum(p[..., 0], q[..., 0])).astype(f32), f32(0))
        height = np.maximum((np.minimum(p[..., 3], q[..., 3]) - np.maximum(p[..., 1], q[..., 1])).astype(f32), f32(0))
        inter = (width * height).astype(f32)
        union = np.maximum(((a1 + a2).astype(f32) - inter).astype(f32), f32(1))
        return (inter / union).astype(f32)


def bbox_overlaps(boxes, query):
    """cython_bbox.pyx:32-73: no +1, zero unless iw > 0 and ih > 0, no union clamp"""
    b, q = boxes.astype(f32)[:, None, :], query.astype(f32)[None, :, :]
    with np.errstate(all="ignore"):
        qa = ((q[..., 2] - q[..., 0]).astype(f32) * (q[..., 3] - q[..., 1]).astype(f32)).astype(f32)
        iw = (np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])).astype(f32)
        ih = (np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])).astype(f32)
        ba = ((b[..., 2] - b[..., 0]).astype(f32) * (b[..., 3] - b[..., 1]).astype(f32)).astype(f32)
        ii = (iw * ih).astype(f32)
        ua = ((ba + qa).astype(f32) - ii).astype(f32)
        return np.where((iw > 0) & (ih > 0), (ii / ua).astype(f32), f32(0)).astype(f32)
