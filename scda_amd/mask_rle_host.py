"""COCO run-length code of ONE boolean mask on the host, in numpy: the rule of include/scda_ops.h (datasets/pycocotools/common/maskApi.c
rleEncode, rleToString, rleArea, rleToBbox).  scda_amd.infer.segm_rows uses it for the detections whose run count exceeded the device
encoder's capacity; tests pin it to the same fixture as the device kernels, so both routes give the same bytes."""
import numpy as np


def rle_counts(mask):
    """bool [h, w] -> uint32 counts: pixels in column-major order (index = x * h + y), the first run counts zeros and may be 0"""
    m = np.asarray(mask, dtype=bool)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("rle_counts: a non-empty [h, w] mask")
    flat = m.T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    head = [0, 0] if flat[0] else [0]
    edges = np.concatenate([np.asarray(head, dtype=np.int64), change.astype(np.int64), np.asarray([flat.size], dtype=np.int64)])
    return np.diff(edges).astype(np.uint32)


def rle_string(counts):
    """rleToString: per run i, x = counts[i] - (i > 2 ? counts[i - 2] : 0); 5 bits per character, low bits first, bit 5 = more follows,
    + 48.  -> str"""
    c0 = np.asarray(counts).astype(np.int64)
    x = c0.copy()
    if len(x) > 3:
        x[3:] = c0[3:] - c0[1:-2]
    chars = np.zeros((len(x), 13), dtype=np.uint8)                     # 13 characters hold any 64-bit value
    alive = np.ones(len(x), dtype=bool)
    used = np.zeros((len(x), 13), dtype=bool)
    for q in range(13):
        c = x & 0x1f
        x = x >> 5
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, q] = (c | (more.astype(np.int64) << 5)) + 48
        used[:, q] = alive
        alive = alive & more
        if not alive.any():
            break
    return chars[used].tobytes().decode('ascii')


def rle_area(counts):
    return int(np.asarray(counts, dtype=np.uint64)[1::2].sum())


def rle_bbox(counts, h):
    """rleToBbox: (x, y, w, h) from the first and last pixel of every run of ones -- a run that wraps into the next column contributes
    only its end points' rows (the reference's behaviour, kept)"""
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0, 0, 0, 0]
    t = np.cumsum(np.asarray(counts[:m], dtype=np.int64)) - (np.arange(m) % 2)
    y = t % h
    x = (t - y) // h
    return [int(x.min()), int(y.min()), int(x.max() - x.min() + 1), int(y.max() - y.min() + 1)]


def encode(mask):
    """bool [h, w] -> {'size': [h, w], 'counts': str, 'area': int, 'bbox': [x, y, w, h]}"""
    m = np.asarray(mask, dtype=bool)
    counts = rle_counts(m)
    return {'size': [int(m.shape[0]), int(m.shape[1])], 'counts': rle_string(counts), 'area': rle_area(counts),
            'bbox': rle_bbox(counts, m.shape[0])}
