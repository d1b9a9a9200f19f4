"""Seeded inputs of the RoI / focal / overlap edge suite, shared by tests/test_roi_refs.py (restatements against the C oracle, CPU) and
tests/test_roi_edges_gpu.py (HIP kernels against the restatements).  numpy only."""
import numpy as np

f32 = np.float32
FLT_MAX = float(np.finfo(f32).max)

# RoI extents (feature pixels) of the sweep; 57, 114 and 121 are the ones whose last 7-bin window ends at extent + 1 in fp32
EXTENTS = list(range(1, 9)) + [13, 14, 15, 56, 57, 58, 113, 114, 115, 120, 121, 122]
SCALE = 1.0 / 16


def sweep_case(axis, clip):
    """-> (features [1,2,8,130] or [1,2,130,8], rois).  Features strictly increase along the long axis and are constant across it.
    RoIs: every extent of EXTENTS along the long axis, starting at 0 and at 5 -- or, with `clip`, starting where ew + 1 == the map's
    size, so that the pixel past the RoI does not exist.  Six pixels (1 .. 6) across."""
    L = 130
    ramp = np.arange(L, dtype=f32)
    feat = np.stack([np.broadcast_to(ramp, (8, L)), np.broadcast_to(2 * ramp + 1, (8, L))])[None].astype(f32)   # [1, 2, 8, 130]
    rois = []
    for e in EXTENTS:
        for s in ([L - e] if clip else [0, 5]):
            rois.append([0, s * 16, 16, (s + e - 1) * 16, 6 * 16])
    rois = np.array(rois, f32)
    if axis == "h":
        feat = np.ascontiguousarray(feat.transpose(0, 1, 3, 2))
        rois = rois[:, [0, 2, 1, 4, 3]]
    return np.ascontiguousarray(feat), np.ascontiguousarray(rois)


def sweep_case_large():
    """[1,1,64,130]: 8320 pixels a plane, past the scatter form's LDS.  Features increase along both axes; widths sweep EXTENTS,
    heights the extents that fit 64 rows."""
    H, W = 64, 130
    feat = (np.arange(W, dtype=f32)[None, :] + W * np.arange(H, dtype=f32)[:, None])[None, None]
    hs = [e for e in EXTENTS if e <= 58]
    rois = []
    for i, e in enumerate(EXTENTS):
        for s in (0, 5):
            eh = hs[(i + s) % len(hs)]
            rois.append([0, s * 16, s * 16, (s + e - 1) * 16, (s + eh - 1) * 16])
    return np.ascontiguousarray(feat, f32), np.array(rois, f32)


def special_pool_cases():
    """-> [(name, features [1,1,8,8], rois)] : special values in the windows, RoIs outside / half outside / inverted / on .5"""
    rs = np.random.RandomState(41)
    base = rs.randn(1, 1, 8, 8).astype(f32)
    H = W = 8
    rois = np.array([
        [0, 0, 0, 127, 127],                       # the whole map
        [0, 16, 16, 63, 63],
        [0, -96, 16, -32, 63],                     # wholly left of the map
        [0, W * 16 + 32, 16, W * 16 + 96, 63],     # right
        [0, 16, -96, 63, -32],                     # above
        [0, 16, H * 16 + 32, 63, H * 16 + 96],     # below
        [0, -48, -48, 47, 47],                     # half outside (up-left)
        [0, 80, 80, 175, 175],                     # half outside (down-right)
        [0, 64, 16, 32, 63],                       # x2 < x1: width 1
        [0, -8, -8, 24, 24],                       # -0.5 -> -1, 1.5 -> 2 (half away from zero)
        [0, 8, 8, 24, 24],                         # 0.5 -> 1
        [0, 24, 24, 24, 24],                       # one pixel: every bin on it
    ], f32)
    cases = [("random", base)]
    cases.append(("constant", np.full_like(base, 2.0)))
    cases.append(("neg_inf", np.full_like(base, -np.inf)))
    cases.append(("neg_flt_max", np.full_like(base, -FLT_MAX)))
    x = base.copy(); x[0, 0, 2, 2] = np.nan; x[0, 0, 0, 0] = np.nan; x[0, 0, 5, 6] = np.nan
    cases.append(("with_nan", x))
    x = base.copy(); x[0, 0, 3, 3] = np.inf; x[0, 0, 3, 5] = np.inf; x[0, 0, 0, 1] = np.nan
    cases.append(("with_pos_inf", x))
    cases.append(("all_nan", np.full_like(base, np.nan)))
    return [(n, np.ascontiguousarray(x), rois) for n, x in cases]


def tied_features(rs, shape):
    feat = rs.randn(*shape).astype(f32)
    feat = (np.round(feat * 2) / 2).astype(f32) + f32(0.0)        # few distinct values: ties in every window; no -0.0
    return feat


def rand_rois(rs, R, B, H, W, scale=SCALE):
    """R RoIs in image coordinates on B maps of H x W: real-valued, integer, on .5 after scaling, tiny, reaching outside"""
    iw, ih = W / scale, H / scale
    x1 = rs.uniform(-0.1 * iw, 0.9 * iw, R); y1 = rs.uniform(-0.1 * ih, 0.9 * ih, R)
    w = np.exp(rs.uniform(np.log(2.0), np.log(iw), R)); h = np.exp(rs.uniform(np.log(2.0), np.log(ih), R))
    b = np.stack([x1, y1, x1 + w, y1 + h], 1)
    q = R // 4
    b[:q] = np.round(b[:q] * scale * 2) / 2 / scale           # halves of a feature pixel: the rounding mode matters
    b[q:q + 3, 2:] = b[q:q + 3, :2] + 1                       # tiny
    bi = rs.randint(0, B, (R, 1))
    return np.concatenate([bi, b], 1).astype(f32)


# ---------------------------------------------------------------- RoIAlign
def align_geometry_rois(H, W):
    """scale 1.0; for 2 x 2 samples the sample rows are y1 and y1 + (y2 - y1 + 1)"""
    below = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))
    return np.array([
        [0, 1, 1, W - 3, H - 3],                   # second sample row exactly on H - 2 ... and
        [0, 1, 1, W - 2, H - 2],                   # exactly on row H - 1 / column W - 1: hstart = H - 2, ratio 1
        [0, below(W), below(H), W + 5, H + 5],     # first sample one ulp below H (ratio 2 - ulp), second outside
        [0, below(0), below(0), 3, 3],             # one ulp below 0: outside
        [0, 0.0, -0.0, 3, 3],                      # on 0 and on -0.0: inside
        [0, 4.25, 2.5, 1.25, 0.5],                 # x2 - x1 + 1 < 0: roi_w, roi_h clamped to 0, every sample on (x1, y1)
        [0, -9, 1, -5, 3], [0, W + 1, 1, W + 4, 3], [0, 1, -9, 3, -5], [0, 1, H + 1, 3, H + 4],    # wholly outside, four sides
        [0, -2.5, -1.5, W + 2.5, H + 1.5],         # reaching out on all sides
    ], f32)


def align_exact_rois(rs, R, B, H, W, AH, AW):
    """scale 1/16.  Corners on multiples of 1/8 feature pixel, roi_w = m (AW - 1) / 8 and roi_h = m' (AH - 1) / 8: every sample
    coordinate and bilinear ratio is a multiple of 1/8, every weight a multiple of 1/64"""
    rois = np.zeros((R, 5), f32)
    rois[:, 0] = rs.randint(0, B, R)
    for r in range(R):
        for k, (L, A) in enumerate(((W, AW), (H, AH))):
            m = rs.randint(1, max(2, int(8 * L / (A - 1))) + 1)      # extent m (A - 1) / 8 pixels: up to about the map
            ext = m * (A - 1) / 8.0
            x1 = rs.randint(-8, 8 * L) / 8.0                          # multiples of 1/8 pixel, some outside
            rois[r, 1 + k] = x1 * 16
            rois[r, 3 + k] = (x1 + ext - 1) * 16
    return rois


def align_inexact_rois(rs, R, B, H, W, pile=0):
    """scale 1/16.  Random geometry; the last `pile` RoIs are one RoI of width and height 0 (all samples on one point)"""
    rois = rand_rois(rs, R, B, H, W)
    if pile:
        rois[R - pile:] = [0, (W / 2 + 0.3) * 16, (H / 2 + 0.6) * 16, (W / 2 + 0.3) * 16 - 16, (H / 2 + 0.6) * 16 - 16]
    return rois


def signed_unit_tops(rs, shape):
    return (rs.uniform(0.5, 1.5, shape) * rs.choice([-1.0, 1.0], shape)).astype(f32)


# ---------------------------------------------------------------- focal losses
EDGE_LOGITS = [0.0, -0.0, 17.0, -17.0, 88.0, -88.0, 100.0, -100.0]


def focal_case(rows, C, softmax, seed=5):
    """-> (logits [rows, C] float32, targets [rows] int32).  The first rows are the edge logits (cyclically), once per target value
    (sigmoid: -1 .. C + 1; softmax: -1 .. C - 1), then rotated so that every target meets every edge value as its own class; then a
    tied row and a row of -100 per target value; random (3 sigma) logits behind; the edge row again in the last row."""
    rs = np.random.RandomState(seed + rows * 131 + C)
    x = (rs.randn(rows, C) * 3).astype(f32)
    labels = list(range(-1, C if softmax else C + 2))
    t = np.array([labels[i % len(labels)] for i in range(rows)], np.int32)
    edge = np.array([EDGE_LOGITS[i % len(EDGE_LOGITS)] for i in range(C + len(EDGE_LOGITS))], f32)
    i = 0
    for shift in range(len(EDGE_LOGITS)):
        for _ in labels:
            if i < rows - 2:
                x[i] = edge[shift:shift + C]; i += 1
    for fill in (1.5, -100.0):
        for _ in labels:
            if i < rows - 2:
                x[i] = fill; i += 1
    x[-1] = edge[:C]
    return x, t


# ---------------------------------------------------------------- overlaps
def overlap_case(n1, n2, sz, seed=9):
    """boxes without the +1 convention: random, touching (iw == 0), zero-area, inverted, tiny (the union clamp at 1)"""
    rs = np.random.RandomState(seed + n1 + n2)

    def boxes(n):
        x1 = rs.uniform(0, 900, n); y1 = rs.uniform(0, 400, n)
        b = np.stack([x1, y1, x1 + np.exp(rs.uniform(0, 5.5, n)), y1 + np.exp(rs.uniform(0, 5, n))], 1)
        b[::3] = np.round(b[::3])
        special = np.array([[10, 10, 20, 20], [20, 10, 30, 20], [10, 20, 20, 30],       # touching the first on x / on y
                            [15, 15, 15, 15], [15, 12, 15, 18],                          # zero area
                            [20, 20, 10, 10], [18, 12, 12, 18],                          # inverted
                            [10, 10, 10.5, 10.5], [10.25, 10.25, 10.75, 10.75],          # union < 1
                            [10, 10, 20, 20]], np.float64)
        k = min(n, len(special))
        b[:k] = special[:k]
        if n > 2 * len(special):
            b[-k:] = special[:k]
        if sz > 4:
            b = np.concatenate([b, rs.uniform(0, 1, (n, sz - 4))], 1)
        return np.ascontiguousarray(b, f32)
    return boxes(n1), boxes(n2)
