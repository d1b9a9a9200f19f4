"""A numpy statement of the rule of scda_mask_frpoly_hip (include/scda_ops.h): the reference's COCO.annToMask -- rleFrPoly, rleMerge
(intersect = 0), frUncompressedRLE / rleFrString and rleDecode of datasets/pycocotools/common/maskApi.c -- said once more as a parity
fill, independent of the product and vectorised over the points of an edge.  tests/test_mask_poly_rules.py pins it to
tests/golden/mask_poly_ref.npz (what the reference's compiled C gives); the GPU test compares the kernel with the same file."""
import numpy as np

INT_MIN = -2 ** 31


def int_vertices(xy):
    """(int)(5 * c + .5): one double multiply, one double add, truncation towards zero.  xy float64 [k, 2] -> int64 [k, 2]"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return np.trunc(5.0 * xy + 0.5).astype(np.int64)


def edge_points(xs, ys, xe, ye):
    """the max(|dx|, |dy|) + 1 points of one edge in the reference's order (maskApi.c:170-179) -> (u, v) int64"""
    dx, dy = abs(xe - xs), abs(ys - ye)
    flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
    if flip:
        xs, xe, ys, ye = xe, xs, ye, ys
    n = max(dx, dy) + 1
    d = np.arange(n, dtype=np.int64)
    t = n - 1 - d if flip else d
    if dx == 0 and dy == 0:                     # s = 0.0 / 0 is NaN and (int)NaN is INT_MIN where the reference was compiled
        return np.array([xs], np.int64), np.array([INT_MIN], np.int64)
    tf = t.astype(np.float64)
    if dx >= dy:
        s = np.float64(ye - ys) / np.float64(dx)
        return t + xs, np.trunc(np.float64(ys) + s * tf + 0.5).astype(np.int64)
    s = np.float64(xe - xs) / np.float64(dy)
    return np.trunc(np.float64(xs) + s * tf + 0.5).astype(np.int64), t + ys


def poly_toggles(xy, h, w):
    """the toggle positions (with repeats) of one polygon in the column-major pixel sequence of an h x w image"""
    p = int_vertices(xy)
    k = len(p)
    if k == 0:
        return np.zeros(0, np.int64)
    us, vs = [], []
    for j in range(k):
        u, v = edge_points(int(p[j, 0]), int(p[j, 1]), int(p[(j + 1) % k, 0]), int(p[(j + 1) % k, 1]))
        us.append(u); vs.append(v)
    u, v = np.concatenate(us), np.concatenate(vs)
    uq, up, vq, vp = u[1:], u[:-1], v[1:], v[:-1]
    cross = uq != up
    xd = np.where(uq < up, uq, uq - 1).astype(np.float64)
    xd = (xd + 0.5) / 5.0 - 0.5
    keep = cross & (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.minimum(vq, vp).astype(np.float64)
    yd = (yd + 0.5) / 5.0 - 0.5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    return (xd[keep].astype(np.int64) * h + yd[keep].astype(np.int64))


def rle_toggles(counts):
    """an uncompressed RLE as toggles: the running sums of its counts; the pixels behind the last run stay 0"""
    c = np.asarray(counts, dtype=np.int64)
    pos = np.cumsum(c)
    return pos if len(c) % 2 == 0 else pos[:-1]


def fill(toggles, h, w):
    """pixel i of the column-major sequence = parity of the toggles at positions <= i -> bool [h, w]"""
    n = h * w
    t = np.asarray(toggles, dtype=np.int64)
    par = np.bincount(t[t < n], minlength=n) & 1
    return (np.cumsum(par) & 1).astype(bool).reshape(w, h).T


def fr_string(s):
    """rleFrString (maskApi.c:217-230): the 6-bit string -> counts (int64)"""
    if isinstance(s, str):
        s = s.encode()
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1; k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xffffffff)
    return np.asarray(cnts, dtype=np.int64)


def annotation(h, w, polygons=(), counts=None):
    """one annotation -> bool [h, w]: the union of its polygons' fills, or the fill of its RLE"""
    m = np.zeros((h, w), dtype=bool)
    for xy in polygons:
        m |= fill(poly_toggles(xy, h, w), h, w)
    if counts is not None:
        m |= fill(rle_toggles(counts), h, w)
    return m


def decode_counts(counts, h, w):
    """rleDecode into a zeroed image -> bool [h, w]"""
    c = np.asarray(counts, dtype=np.int64)
    flat = np.zeros(h * w, dtype=bool)
    vals = np.repeat(np.arange(len(c)) % 2 == 1, c)
    flat[:len(vals)] = vals
    return flat.reshape(w, h).T
