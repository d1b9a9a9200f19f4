"""A numpy statement of the rules of scda_mask_rle_hip / scda_mask_iou_hip (include/scda_ops.h): the reference's
datasets/pycocotools/common/maskApi.c rleEncode, rleToString, rleArea, rleToBbox, bbIou and rleIou said once more, independent of the
product.  tests/test_mask_rle_rules.py pins it to tests/golden/mask_rle_ref.npz (what the reference's compiled C gives); the GPU tests
then use it where the fixture has no case."""
import numpy as np


def unpack(words, h, w):
    """uint32 / int32 [..., H, Wd] words -> bool [..., h, w]: bit (c % 32) of word c // 32, cropped to the image"""
    u8 = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(u8, axis=-1, bitorder='little')[..., :h, :w].astype(bool)


def encode(mask):
    """rleEncode of bool [h, w] -> uint32 counts.  The pixels are walked column by column; a run ends where the value changes; the first
    run is of zeros (length 0 if the first pixel is set)"""
    t = np.asarray(mask).astype(np.uint8).flatten(order='F')
    prev = np.concatenate([[0], t[:-1]]).astype(np.uint8)                # p = 0 before the first pixel
    starts = np.flatnonzero(t != prev)                                    # a new run starts here
    bounds = np.concatenate([[0], starts, [t.size]])
    return (bounds[1:] - bounds[:-1]).astype(np.uint32)


def to_string(counts):
    """rleToString -> bytes"""
    c = np.asarray(counts, dtype=np.int64)
    x = c.copy()
    x[3:] -= c[1:-2]
    out = np.zeros((len(x), 14), dtype=np.uint8)
    length = np.zeros(len(x), dtype=np.int64)
    more = np.ones(len(x), dtype=bool)
    for k in range(14):
        if not more.any():
            break
        ch = x & 0x1f
        x = x >> 5                                                        # arithmetic shift on int64
        nxt = np.where(ch & 0x10, x != -1, x != 0)
        ch = np.where(nxt, ch | 0x20, ch) + 48
        out[more, k] = ch[more]
        length[more] += 1
        more = more & nxt
    keep = np.arange(14)[None, :] < length[:, None]
    return out[keep].tobytes()


def area(counts):
    return int(np.asarray(counts, dtype=np.int64)[1::2].sum())


def to_bbox(counts, h):
    """rleToBbox from the run end points (maskApi.c:133-146) -> [x, y, w, h]"""
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0, 0, 0, 0]
    cc = np.cumsum(np.asarray(counts[:m], dtype=np.int64))
    t = cc - (np.arange(m) % 2)
    y = t % h
    x = (t - y) // h
    return [int(x.min()), int(y.min()), int(x.max() - x.min() + 1), int(y.max() - y.min() + 1)]


def statement(mask):
    """every output of rule (a) for one bool [h, w] mask"""
    counts = encode(mask)
    return {'n_runs': len(counts), 'counts': counts, 'chars': to_string(counts), 'area': area(counts),
            'bbox': to_bbox(counts, np.asarray(mask).shape[0])}


def iou(dt, gt, iscrowd=None):
    """rule (b): dt bool [M, h, w], gt bool [N, h, w] -> (o float64 [N, M], inter uint32 [N, M])"""
    dt, gt = np.asarray(dt, dtype=bool), np.asarray(gt, dtype=bool)
    M, N = dt.shape[0], gt.shape[0]
    h = dt.shape[1]
    db = [to_bbox(encode(m), h) for m in dt]
    gb = [to_bbox(encode(m), h) for m in gt]
    o = np.zeros((N, M), dtype=np.float64)
    inter = np.zeros((N, M), dtype=np.uint32)
    for g in range(N):
        for d in range(M):
            i = int((dt[d] & gt[g]).sum())
            inter[g, d] = i
            D, G = db[d], gb[g]
            bw = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            bh = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if bw <= 0 or bh <= 0 or i == 0:
                continue
            crowd = iscrowd is not None and bool(iscrowd[g])
            u = int(dt[d].sum()) if crowd else int(dt[d].sum()) + int(gt[g].sum()) - i
            o[g, d] = np.float64(i) / np.float64(u)
    return o, inter
