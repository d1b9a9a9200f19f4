"""Plain torch restatements of the convolution, Winograd and GEMM kernels (scda_amd/csrc/conv_gemm.hip, conv_wino.hip), the dtype a
parameter: float64 is the reference of tests/test_conv_edges_gpu.py, float32 the same algorithm at the kernels' precision.
tests/test_conv_refs.py checks them on the CPU.

Every function returns (value, S): S is the element-wise magnitude sum, the same operation on absolute operands -- sum |a||b| + |bias|
(+ |previous out| when accumulating): what round-off of any summation order is proportional to.  The Winograd functions return S_w,
the magnitude sum of the transform chain itself (|G|, |B|, |A| and absolute operands); S_w >= S element-wise."""
import contextlib

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def apply_act(t, act, slope):
    if act == ACT_RELU:
        return torch.where(t > 0, t, torch.zeros_like(t))
    if act == ACT_LEAKY:
        return torch.where(t > 0, t, t * slope)
    return t


def act_mask(src, slope, dtype):
    """the activation gradient of the layer that produced src: 1 where src > 0, else slope"""
    return torch.where(src > 0, torch.ones((), dtype=dtype), torch.full((), slope, dtype=dtype)).to(dtype)


def offset_view(t, device):
    """t on the device as a CONTIGUOUS view one element into a larger buffer: 4 bytes off every 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# ------------------------------------------------------------------ direct form
def _fwd(x, w, bias, stride, pad):
    return F.conv2d(x, w, bias, stride=stride, padding=pad)


def conv_fwd(x, w, bias, stride, pad, act=ACT_NONE, slope=0.01, dtype=torch.float64):
    x, w = x.to(dtype), w.to(dtype)
    b = None if bias is None else bias.to(dtype)
    y = apply_act(_fwd(x, w, b, stride, pad), act, slope)
    S = _fwd(x.abs(), w.abs(), None if b is None else b.abs(), stride, pad)
    return y, S


def _dgrad(dy, w, x_shape, stride, pad):
    KH, KW = w.shape[2:]
    oph = x_shape[2] - ((dy.shape[2] - 1) * stride - 2 * pad + KH)
    opw = x_shape[3] - ((dy.shape[3] - 1) * stride - 2 * pad + KW)
    return F.conv_transpose2d(dy, w, None, stride=stride, padding=pad, output_padding=(oph, opw))


def conv_dgrad(dy, w, x_shape, stride, pad, act_src=None, act_slope=0.0, dtype=torch.float64):
    dy, w = dy.to(dtype), w.to(dtype)
    dx, S = _dgrad(dy, w, x_shape, stride, pad), _dgrad(dy.abs(), w.abs(), x_shape, stride, pad)
    if act_src is not None:
        m = act_mask(act_src, act_slope, dtype)
        dx, S = dx * m, S * m.abs()
    return dx, S


def _wgrad(dy, x, w_shape, stride, pad):
    return torch.nn.grad.conv2d_weight(x, tuple(w_shape), dy, stride=stride, padding=pad)


def conv_wgrad(dy, x, w_shape, stride, pad, prev=None, prev_db=None, dtype=torch.float64):
    """-> ((dw, db), (S_dw, S_db)); prev / prev_db: the gradients already in the buffers the kernel accumulates into"""
    dy, x = dy.to(dtype), x.to(dtype)
    dw, S = _wgrad(dy, x, w_shape, stride, pad), _wgrad(dy.abs(), x.abs(), w_shape, stride, pad)
    db, Sb = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
    if prev is not None:
        dw, S = dw + prev.to(dtype), S + prev.to(dtype).abs()
    if prev_db is not None:
        db, Sb = db + prev_db.to(dtype), Sb + prev_db.to(dtype).abs()
    return (dw, db), (S, Sb)


# ---- row_period stacks: [1, C, R * 7, 7] as R independent 7 x 7 maps
def unstack(t, period=7):
    """[1, C, R * p, W] -> [R, C, p, W]"""
    C, W = t.shape[1], t.shape[3]
    return t.reshape(C, t.shape[2] // period, period, W).permute(1, 0, 2, 3).contiguous()


def stack(t):
    """[R, C, p, W] -> [1, C, R * p, W]"""
    R, C, p, W = t.shape
    return t.permute(1, 0, 2, 3).reshape(1, C, R * p, W).contiguous()


def stacked_fwd(x, w, bias, act=ACT_NONE, slope=0.01, dtype=torch.float64, period=7):
    y, S = conv_fwd(unstack(x, period), w, bias, 1, w.shape[2] // 2, act, slope, dtype)
    return stack(y), stack(S)


def stacked_dgrad(dy, w, act_src=None, act_slope=0.0, dtype=torch.float64, period=7):
    d = unstack(dy, period)
    src = None if act_src is None else unstack(act_src, period)
    dx, S = conv_dgrad(d, w, (d.shape[0], w.shape[1], d.shape[2], d.shape[3]), 1, w.shape[2] // 2, src, act_slope, dtype)
    return stack(dx), stack(S)


def stacked_wgrad(dy, x, w_shape, prev=None, prev_db=None, dtype=torch.float64, period=7):
    return conv_wgrad(unstack(dy, period), unstack(x, period), w_shape, 1, w_shape[2] // 2, prev, prev_db, dtype)


# ---- dense GEMM, the four operand layouts (include/scda_ops.h: trans_a: A stored [K][M], trans_b: B stored [K][N])
def gemm(a, b, trans_a=False, trans_b=False, bias=None, bias_on_n=True, act=ACT_NONE, slope=0.01, prev=None, dtype=torch.float64):
    """C[M, N] = op(A) op(B) (+ bias) -> act (+ prev); without trans_b B is stored [N][K] (an nn.Linear weight)"""
    A = a.to(dtype).t() if trans_a else a.to(dtype)
    Bm = b.to(dtype) if trans_b else b.to(dtype).t()
    c, S = A @ Bm, A.abs() @ Bm.abs()
    if bias is not None:
        bb = bias.to(dtype)
        bb = bb[None, :] if bias_on_n else bb[:, None]
        c, S = c + bb, S + bb.abs()
    c = apply_act(c, act, slope)
    if prev is not None:
        c, S = c + prev.to(dtype), S + prev.to(dtype).abs()
    return c, S


# ------------------------------------------------------------------ Winograd F(2x2, 3x3)
#   Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A     per 2 x 2 output tile, 4 x 4 input tile d, 3 x 3 filter g
WG = [[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]]
WBT = [[1.0, 0.0, -1.0, 0.0], [0.0, 1.0, 1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [0.0, 1.0, 0.0, -1.0]]
WAT = [[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]]


def _mats(dtype, absolute):
    ms = [torch.tensor(m, dtype=dtype) for m in (WG, WBT, WAT)]
    return [m.abs() for m in ms] if absolute else ms


def _patches(x):
    """[B, C, H, W] (even H, W), zero padding 1 -> [B, C, H/2, W/2, 4, 4]: the 4 x 4 input tile of every 2 x 2 output tile"""
    return F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)


def _tiles(y):
    """[B, M, H, W] -> [B, M, H/2, W/2, 2, 2]"""
    return y.unfold(2, 2, 2).unfold(3, 2, 2)


def _untile(t):
    B, M, th, tw = t.shape[:4]
    return t.permute(0, 1, 2, 4, 3, 5).reshape(B, M, th * 2, tw * 2)


def _wino_chain(x, w, absolute):
    G, BT, AT = _mats(x.dtype, absolute)
    U = torch.einsum("ij,mcjk,lk->mcil", G, w, G)                     # G g G^T
    V = torch.einsum("ij,bcxyjk,lk->bcxyil", BT, _patches(x), BT)     # B^T d B
    Mx = torch.einsum("mcil,bcxyil->bmxyil", U, V)
    return _untile(torch.einsum("ij,bmxyjk,lk->bmxyil", AT, Mx, AT))  # A^T . A


def wino_fwd(x, w, bias, act=ACT_NONE, slope=0.01, dtype=torch.float64):
    x, w = x.to(dtype), w.to(dtype)
    y, S = _wino_chain(x, w, False), _wino_chain(x.abs(), w.abs(), True)
    if bias is not None:
        b = bias.to(dtype)[None, :, None, None]
        y, S = y + b, S + b.abs()
    return apply_act(y, act, slope), S


def wino_dgrad(dy, w, act_src=None, act_slope=0.0, dtype=torch.float64):
    """the data gradient of a stride-1 pad-1 3x3 layer is the same convolution with rotated, channel-swapped filters"""
    wr = w.to(dtype).transpose(0, 1).flip(2, 3).contiguous()
    dx, S = _wino_chain(dy.to(dtype), wr, False), _wino_chain(dy.to(dtype).abs(), wr.abs(), True)
    if act_src is not None:
        m = act_mask(act_src, act_slope, dtype)
        dx, S = dx * m, S * m.abs()
    return dx, S


def _wino_wgrad_chain(dy, x, absolute):
    """dg[m][c] = G^T [ sum_t (A dY_t A^T) .* (B^T d_t B) ] G: the transposed bilinear algorithm (head of conv_wino_wgrad_kernel)"""
    G, BT, AT = _mats(x.dtype, absolute)
    Z = torch.einsum("ji,bmxyjk,kl->bmxyil", AT, _tiles(dy), AT)      # A dY A^T (A = AT^T)
    V = torch.einsum("ij,bcxyjk,lk->bcxyil", BT, _patches(x), BT)
    dU = torch.einsum("bmxyil,bcxyil->mcil", Z, V)
    return torch.einsum("ji,mcjk,kl->mcil", G, dU, G)                 # G^T . G


def wino_wgrad(dy, x, prev=None, prev_db=None, dtype=torch.float64):
    dy, x = dy.to(dtype), x.to(dtype)
    dw, S = _wino_wgrad_chain(dy, x, False), _wino_wgrad_chain(dy.abs(), x.abs(), True)
    db, Sb = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
    if prev is not None:
        dw, S = dw + prev.to(dtype), S + prev.to(dtype).abs()
    if prev_db is not None:
        db, Sb = db + prev_db.to(dtype), Sb + prev_db.to(dtype).abs()
    return (dw, db), (S, Sb)


# the kernels run a stack of 7 x 7 maps as 8 x 8 maps whose last row / column is discarded: the same chain on the padded map
def _pad8(t):
    return F.pad(t, (0, 1, 0, 1))


def wino_stacked_fwd(x, w, bias, act=ACT_NONE, slope=0.01, dtype=torch.float64):
    y, S = wino_fwd(_pad8(unstack(x)), w, bias, act, slope, dtype)
    return stack(y[:, :, :7, :7]), stack(S[:, :, :7, :7])


def wino_stacked_dgrad(dy, w, act_src=None, act_slope=0.0, dtype=torch.float64):
    src = None if act_src is None else _pad8(unstack(act_src))
    dx, S = wino_dgrad(_pad8(unstack(dy)), w, src, act_slope, dtype)
    return stack(dx[:, :, :7, :7]), stack(S[:, :, :7, :7])


def wino_stacked_wgrad(dy, x, prev=None, prev_db=None, dtype=torch.float64):
    return wino_wgrad(_pad8(unstack(dy)), _pad8(unstack(x)), prev, prev_db, dtype)


# ------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, seed):
    """float32 integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen(seed)).float()


def gauss(shape, seed, kind="gauss"):
    """full-mantissa float32 inputs: zero-mean Gaussian, post-ReLU (half zeros), or mean 100 / std 1 (no cancellation, large S)"""
    t = torch.randn(tuple(shape), generator=gen(seed))
    return t.clamp_min(0) if kind == "relu" else t + 100.0 if kind == "mean100" else t


# ------------------------------------------------------------------ the edge shapes (tests/test_conv_edges_gpu.py, test_conv_refs.py)
# Direct implicit-GEMM family (SCDA_WINOGRAD=0).  name, B, Cin, H, W, Cout, k, stride, pad, row_period, forced (bm, bn, splits) of
# the forward / data-gradient launch (of the weight gradient where that is the only direction) or None, directions (f forward, d data gradient, w weight + bias gradient)
def _seams():
    """pixel counts of tile - 1, tile, tile + 1 for the tile widths 64 / 128 / 256 (16 -> 16 channels: every width is legal on the 64-row
    tile), several images per tile where the count factors: image seams inside the tile; unsplit and split in two (both reduce forms:
    four-pixel groups need N % 4 == 0 and H W % 4 == 0)"""
    shapes = {63: (3, 3, 7), 64: (2, 4, 8), 65: (5, 1, 13), 127: (1, 1, 127), 128: (2, 8, 8), 129: (3, 1, 43), 255: (3, 5, 17),
              256: (4, 8, 8), 257: (1, 1, 257)}
    out = []
    for bn in (64, 128, 256):
        for n in (bn - 1, bn, bn + 1):
            B, H, W = shapes[n]
            for sp in (1, 2):
                out.append(("seam%d_n%d_s%d" % (bn, n, sp), B, 16, H, W, 16, 3, 1, 1, 0, (64, bn, sp), "fdw"))
    return out


DIRECT_CASES = [
    ("map1x1", 1, 16, 1, 1, 16, 3, 1, 1, 0, None, "fdw"),          # 3x3 pad 1 on one pixel: the centre tap only
    ("map1xW", 1, 16, 1, 9, 17, 3, 1, 1, 0, None, "fdw"),
    ("mapHx1", 2, 17, 9, 1, 16, 3, 1, 1, 0, None, "fdw"),
    ("map2x2", 1, 15, 2, 2, 15, 3, 1, 1, 0, None, "fdw"),
    ("one_output", 1, 16, 3, 3, 1, 3, 1, 0, 0, None, "fdw"),       # 3x3 pad 0 on a 3x3 map; Cout 1
    ("s2_map1x1", 2, 16, 1, 1, 33, 3, 2, 1, 0, None, "fdw"),
    ("s2_map2x3", 1, 1, 2, 3, 16, 3, 2, 1, 0, None, "fdw"),        # Cin 1
    ("s2_odd", 1, 16, 3, 5, 16, 3, 2, 1, 0, None, "fdw"),          # stride-2 data gradient without parity classes (odd extents)
    ("s2_parity", 2, 16, 4, 6, 16, 3, 2, 1, 0, None, "fdw"),       # ... by parity classes, an image seam inside each class
    ("s2_parity_split", 2, 16, 4, 6, 64, 3, 2, 1, 0, (64, 64, 2), "fd"),
    ("stem7x7", 1, 3, 4, 4, 64, 7, 2, 3, 0, None, "f"),
    ("k1_one_slab", 1, 16, 4, 4, 17, 1, 1, 0, 0, None, "fdw"),     # K = 16: a single K-slab
    ("k1_stride2", 2, 32, 5, 7, 16, 1, 2, 0, 0, None, "fdw"),
    ("cin1", 1, 1, 4, 5, 17, 3, 1, 1, 0, None, "fdw"),
    ("cout1_gather", 2, 17, 3, 5, 1, 3, 1, 1, 0, None, "fdw"),     # dw has 153 elements: the scalar reduce's tail of 1
    ("small_cin", 1, 3, 2, 65, 5, 3, 1, 1, 0, None, "fdw"),        # image-side kernels (rows of 65: one pixel over the strip of 64)
    ("split_tail", 1, 16, 1, 9, 17, 3, 1, 1, 0, (64, 64, 2), "fd"),   # 17 x 9 = 153 outputs through the scalar conv reduce
    ("tile32_cout1", 2, 16, 5, 13, 1, 3, 1, 1, 0, (32, 256, 1), "f"),
    ("tile32_cout32", 1, 16, 1, 257, 32, 3, 1, 1, 0, (32, 256, 1), "fd"),
    ("tile128x128", 1, 80, 3, 43, 80, 3, 1, 1, 0, (128, 128, 1), "fd"),
    ("tile128x64_split", 1, 80, 3, 43, 80, 3, 1, 1, 0, (128, 64, 3), "fd"),
    ("tile64_on_80rows", 1, 80, 3, 43, 80, 3, 1, 1, 0, (64, 64, 1), "fd"),      # SCDA_PLAN_ALLOW_BM64
    ("tile256x128", 1, 16, 3, 43, 256, 3, 1, 1, 0, (256, 128, 1), "f"),
    ("gather128x128", 1, 15, 3, 43, 65, 3, 1, 1, 0, (128, 128, 1), "f"),
    ("gather64x128_split", 1, 15, 3, 43, 33, 3, 1, 1, 0, (64, 128, 2), "f"),
    ("gather128x64", 1, 15, 3, 43, 65, 3, 1, 1, 0, (128, 64, 1), "f"),
    ("wgrad_one_partial_slab", 1, 16, 3, 3, 16, 3, 1, 1, 0, None, "w"),         # K = 9 pixels
    ("wgrad_27_pixels", 3, 16, 3, 3, 33, 3, 1, 1, 0, None, "w"),                # B H W no multiple of 4
    ("wgrad_vec4", 1, 16, 2, 6, 16, 3, 1, 1, 0, None, "w"),                     # 12 pixels: register-staged with float4 dy loads
    ("wgrad_lds_dma", 2, 16, 4, 4, 33, 3, 1, 1, 0, None, "w"),                  # 16-pixel planes: LDS-DMA + the fused bias gradient
    ("wgrad_lds_dma_tile32", 2, 16, 4, 8, 8, 3, 1, 1, 0, None, "w"),            # <= 32 output channels: the 32 x 128 tile
    ("wgrad_lds_dma_cout1", 2, 16, 4, 8, 1, 3, 1, 1, 0, None, "w"),
    ("wgrad_lds_dma_128rows", 1, 16, 4, 4, 80, 3, 1, 1, 0, None, "w"),
    ("wgrad_lds_dma_256rows", 1, 16, 4, 4, 256, 3, 1, 1, 0, None, "w"),
    ("wgrad_staged_128rows", 1, 16, 3, 5, 80, 3, 1, 1, 0, None, "w"),
    ("wgrad_8_splits", 2, 16, 16, 16, 17, 3, 1, 1, 0, (64, 128, 8), "w"),       # the reduce's four-group form (8 .. 31 slabs); dy offset: register-staged
    ("wgrad_32_splits", 2, 16, 32, 32, 17, 3, 1, 1, 0, (64, 128, 32), "w"),     # ... and its eight-group form
    ("stack1", 1, 16, 7, 7, 16, 3, 1, 1, 7, None, "fdw"),
    ("stack3", 1, 16, 21, 7, 17, 3, 1, 1, 7, None, "fdw"),
    ("stack4", 1, 16, 28, 7, 16, 3, 1, 1, 7, None, "fdw"),
    ("stack5", 1, 15, 35, 7, 16, 3, 1, 1, 7, None, "fdw"),
] + _seams()

# Winograd kernels, called directly (native.conv2d_wino / conv2d_wino_wgrad).  name, B, C (reduced channels), H, W, M (output rows),
# stacked maps (0: a plain image), environment, directions (f forward, d data gradient -- x is dy, C = Cout, M = Cin --, w weight
# gradient with Cin = C, Cout = M), expected (persistent, gm, splits) of the forward launch / expected splits of the weight gradient
WINO_CASES = [
    ("map2x2_m1", 1, 8, 2, 2, 1, 0, {}, "f", (False, 1, 1)),                    # one slab, one output row
    ("map2x32_m65", 1, 8, 2, 32, 65, 0, {}, "f", (False, 1, 1)),
    ("map8x2_m33", 2, 16, 8, 2, 33, 0, {}, "f", (False, 1, 1)),                 # the 32-row tile with one row in its second tile
    ("partial_block", 1, 16, 6, 20, 24, 0, {}, "fd", (False, 1, 1)),
    ("auto_split", 1, 64, 8, 32, 64, 0, {}, "fd", (False, 1, 2)),
    ("forced_split", 1, 16, 8, 34, 64, 0, {"SCDA_WINO_SPLITS": "2"}, "fd", (False, 1, 2)),
    ("xcd_split", 1, 8, 32, 256, 128, 0, {"SCDA_WINO_GM": "2"}, "f", (False, 2, 1)),
    ("persistent", 1, 16, 2, 8222, 64, 0, {}, "fd", (True, 1, 1)),              # 257 tiles of 64 rows, the last block 30 columns wide
    ("one_tile_per_wg", 1, 16, 2, 8222, 64, 0, {"SCDA_WINO_PERSIST": "0"}, "f", (False, 1, 1)),
    ("wgrad_partial_slab", 1, 32, 2, 6, 40, 0, {}, "w", 1),
    ("wgrad_splits1", 1, 32, 16, 64, 72, 0, {"SCDA_WINO_WGRAD_SPLITS": "1"}, "w", 1),
    ("wgrad_splits2", 1, 32, 16, 64, 72, 0, {"SCDA_WINO_WGRAD_SPLITS": "2"}, "w", 2),
    ("wgrad_splits4", 1, 32, 16, 64, 72, 0, {"SCDA_WINO_WGRAD_SPLITS": "4"}, "w", 4),
    ("wgrad_splits8", 1, 32, 16, 128, 40, 0, {"SCDA_WINO_WGRAD_SPLITS": "8"}, "w", 8),      # whole runs of splits per XCD
    ("wgrad_two_images", 2, 40, 4, 18, 32, 0, {}, "w", 1),
    ("stack1", 1, 64, 7, 7, 64, 1, {}, "fdw", (False, 1, None)),
    ("stack3", 1, 64, 21, 7, 64, 3, {}, "fdw", (False, 1, None)),
    ("stack4", 1, 64, 28, 7, 72, 4, {}, "fdw", (False, 1, None)),
    ("stack5", 1, 64, 35, 7, 64, 5, {}, "fdw", (False, 1, None)),
]

# Dense GEMM: name, M, N, K, forced plan, environment; every case runs in the four operand layouts
GEMM_CASES = [
    ("one", 1, 1, 1, None, {}),
    ("row_k17", 1, 4096, 17, None, {}),
    ("m65_n129_k16", 65, 129, 16, None, {}),
    ("split2", 64, 64, 64, (64, 64, 2), {}),
    ("split3_m33", 33, 20, 96, (64, 64, 3), {}),
    ("split8", 33, 20, 256, (64, 64, 8), {}),                   # the reduce's four-group and eight-group forms
    ("split32", 20, 12, 1024, (64, 64, 32), {}),
    ("tile128x128", 132, 136, 32, (128, 128, 1), {}),
    ("tile64x128", 40, 136, 32, (64, 128, 1), {}),
    ("tile128x64", 132, 40, 32, (128, 64, 1), {}),
    ("tile256x128", 256, 136, 32, (256, 128, 1), {}),
    ("x9_k16", 65, 129, 16, None, {"SCDA_GEMM_X9": "2"}),
    ("x9_split2", 260, 132, 64, None, {"SCDA_GEMM_X9": "2", "SCDA_GEMM_X9_SPLITS": "2"}),
    ("x9_stream", 260, 132, 64, None, {"SCDA_GEMM_X9": "2", "SCDA_GEMM_X9_SK": "2"}),
]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]

INT_X, INT_W = 4, 3          # integer operands: activations / gradients in [-4, 4], weights, bias and previous outputs in [-3, 3]


def direct_data(case, kind, seed=0):
    """operands of a DIRECT_CASES / WINO_CASES-shaped layer: kind "int" (small integers) or a gauss() kind"""
    name, B, Cin, H, W, Cout, k, s, p = case[:9]
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    shapes = dict(x=(B, Cin, H, W), w=(Cout, Cin, k, k), bias=(Cout,), dy=(B, Cout, OH, OW), src=(B, Cin, H, W), prev=(Cout, Cin, k, k),
                  prev_db=(Cout,))
    d = {}
    for i, (key, shape) in enumerate(shapes.items()):
        if kind == "int":
            d[key] = ints(shape, -INT_X, INT_X, seed * 16 + i) if key in ("x", "dy", "src") else ints(shape, -INT_W, INT_W, seed * 16 + i)
        else:
            d[key] = gauss(shape, seed * 16 + i, "gauss" if key in ("w", "bias", "src", "prev", "prev_db") else kind)
            if key == "w":
                d[key] = d[key] / (Cin * k * k) ** 0.5
    return d


def direct_refs(case, d):
    """operation name -> f(dtype) -> (value, S) (weight gradient: ((dw, db), (S_dw, S_db))) for the directions of a DIRECT_CASES entry"""
    name, B, Cin, H, W, Cout, k, s, p, rp, force, dirs = case
    xs, ws = d["x"].shape, d["w"].shape
    r = {}
    if rp:
        fwd = lambda bias, act, sl: (lambda dt: stacked_fwd(d["x"], d["w"], bias, act, sl, dt, rp))
        dgr = lambda src, sl: (lambda dt: stacked_dgrad(d["dy"], d["w"], src, sl, dt, rp))
        wgr = lambda pv, pb: (lambda dt: stacked_wgrad(d["dy"], d["x"], ws, pv, pb, dt, rp))
    else:
        fwd = lambda bias, act, sl: (lambda dt: conv_fwd(d["x"], d["w"], bias, s, p, act, sl, dt))
        dgr = lambda src, sl: (lambda dt: conv_dgrad(d["dy"], d["w"], xs, s, p, src, sl, dt))
        wgr = lambda pv, pb: (lambda dt: conv_wgrad(d["dy"], d["x"], ws, s, p, pv, pb, dt))
    if "f" in dirs:
        r["fwd"], r["fwd_relu"], r["fwd_leaky"] = fwd(None, ACT_NONE, 0.0), fwd(d["bias"], ACT_RELU, 0.0), fwd(d["bias"], ACT_LEAKY, 0.25)
    if "d" in dirs:
        r["dgrad"], r["dgrad_mask"] = dgr(None, 0.0), dgr(d["src"], 0.5)
    if "w" in dirs:
        r["wgrad"], r["wgrad_acc"] = wgr(None, None), wgr(d["prev"], d["prev_db"])
    return r


def wino_data(case, kind, seed=0):
    """x [B, C, H, W] is the gathered tensor of every direction (the data gradient's dy); w_f [M, C, 3, 3] the forward's filters, w_d
    [C, M, 3, 3] the data gradient's (Cout = C, Cin = M); dy [B, M, H, W] the weight gradient's output gradient"""
    name, B, C, H, W, M = case[:6]
    shapes = dict(x=(B, C, H, W), w_f=(M, C, 3, 3), bias=(M,), w_d=(C, M, 3, 3), src=(B, M, H, W), dy=(B, M, H, W), prev=(M, C, 3, 3),
                  prev_db=(M,))
    d = {}
    for i, (key, shape) in enumerate(shapes.items()):
        if kind == "int":
            d[key] = ints(shape, -INT_X, INT_X, seed * 16 + i) if key in ("x", "dy", "src") else ints(shape, -INT_W, INT_W, seed * 16 + i)
        else:
            d[key] = gauss(shape, seed * 16 + i, kind if key in ("x", "dy") else "gauss")
            if key in ("w_f", "w_d"):
                d[key] = d[key] / (C * 9) ** 0.5
    return d


def wino_refs(case, d, direct=False):
    name, B, C, H, W, M, maps, env, dirs, expect = case
    if maps:
        fwd, dgr, wgr = (stacked_fwd, stacked_dgrad, lambda dy, x, pv, pb, dt: stacked_wgrad(dy, x, (M, C, 3, 3), pv, pb, dt)) if direct else \
            (wino_stacked_fwd, wino_stacked_dgrad, wino_stacked_wgrad)
    elif direct:
        fwd = lambda x, w, b, act, sl, dt: conv_fwd(x, w, b, 1, 1, act, sl, dt)
        dgr = lambda dy, w, src, sl, dt: conv_dgrad(dy, w, (B, M, H, W), 1, 1, src, sl, dt)
        wgr = lambda dy, x, pv, pb, dt: conv_wgrad(dy, x, (M, C, 3, 3), 1, 1, pv, pb, dt)
    else:
        fwd, dgr, wgr = wino_fwd, wino_dgrad, wino_wgrad
    r = {}
    if "f" in dirs:
        r["fwd_relu"] = lambda dt: fwd(d["x"], d["w_f"], d["bias"], ACT_RELU, 0.0, dt)
        r["fwd_leaky"] = lambda dt: fwd(d["x"], d["w_f"], d["bias"], ACT_LEAKY, 0.25, dt)
    if "d" in dirs:
        r["dgrad"] = lambda dt: dgr(d["x"], d["w_d"], None, 0.0, dt)
        r["dgrad_mask"] = lambda dt: dgr(d["x"], d["w_d"], d["src"], 0.5, dt)
    if "w" in dirs:
        r["wgrad"] = lambda dt: wgr(d["dy"], d["x"], None, None, dt)
        r["wgrad_acc"] = lambda dt: wgr(d["dy"], d["x"], d["prev"], d["prev_db"], dt)
    return r


def gemm_data(case, ta, tb, kind, seed=0):
    name, M, N, K = case[:4]
    mk = (lambda shape, i, r: ints(shape, -r, r, seed * 8 + i)) if kind == "int" else (lambda shape, i, r: gauss(shape, seed * 8 + i, kind if i == 0 else "gauss"))
    a, b = mk((M, K), 0, INT_X), mk((N, K), 1, INT_W)
    if kind != "int":
        b = b / K ** 0.5
    return dict(a=a.t().contiguous() if ta else a, b=b.t().contiguous() if tb else b, bias=mk((N,), 2, INT_W), bias_m=mk((M,), 3, INT_W),
                prev=mk((M, N), 4, INT_W))


def gemm_refs(d, ta, tb):
    return {"plain": lambda dt: gemm(d["a"], d["b"], ta, tb, dtype=dt),
            "bias_relu": lambda dt: gemm(d["a"], d["b"], ta, tb, d["bias"], True, ACT_RELU, 0.0, dtype=dt),
            "bias_m_leaky": lambda dt: gemm(d["a"], d["b"], ta, tb, d["bias_m"], False, ACT_LEAKY, 0.25, dtype=dt),
            "accumulate": lambda dt: gemm(d["a"], d["b"], ta, tb, prev=d["prev"], dtype=dt)}


@contextlib.contextmanager
def plan_env(monkeypatch, force, name, env=None):
    """the switches of one case for the length of a with-block: SCDA_PLAN_FORCE (+ SCDA_PLAN_ALLOW_BM64 for the 64-row tile on a taller
    problem) and its own; monkeypatch: the fixture, or pytest.MonkeyPatch itself"""
    with monkeypatch.context() as m:
        if force:
            m.setenv("SCDA_PLAN_FORCE", "%d,%d,%d" % force)
            if name == "tile64_on_80rows":
                m.setenv("SCDA_PLAN_ALLOW_BM64", "1")
        for key, val in (env or {}).items():
            m.setenv(key, val)
        yield
