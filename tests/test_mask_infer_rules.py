"""The rule of the device mask paste (scda_amd/csrc/mask_ops.hip, include/scda_ops.h), restated in numpy, is Pillow's float resize bit
for bit and reproduces the reference's predict_masks (functions/mask.py:21-49) in the golden fixtures; the bit packing restated.
CPU only.  The device kernels implement exactly these statements (tests/test_mask_infer_gpu.py compares them)."""
import os

import numpy as np
import pytest

import mask_cases as mcases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_taps(n_in, n_out):
    """per output index of an axis n_in -> n_out: (first tap, normalised float64 weights), as Pillow's precompute_coeffs builds them
    for BICUBIC over the whole axis.  Python floats are IEEE doubles and every operator below is one operation."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [bicubic((k + xmin - center + 0.5) * ss) for k in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, w))
    return out


def resize_last_axis(img, n_out):
    """img float32 [rows, n_in] -> float32 [rows, n_out]; equal sizes: the pass is skipped"""
    n_in = img.shape[1]
    if n_in == n_out:
        return img
    out = np.empty((img.shape[0], n_out), dtype=np.float32)
    for xx, (xmin, w) in enumerate(axis_taps(n_in, n_out)):
        s = np.zeros(img.shape[0], dtype=np.float64)
        for k, v in enumerate(w):                       # left to right, (double)pixel * weight
            s = s + img[:, xmin + k].astype(np.float64) * v
        out[:, xx] = s.astype(np.float32)
    return out


def resize_plane(plane, out_w, out_h):
    """rule c's resize: the horizontal pass into a float32 intermediate, then the vertical pass"""
    tmp = resize_last_axis(np.ascontiguousarray(plane, dtype=np.float32), out_w)
    return np.ascontiguousarray(resize_last_axis(np.ascontiguousarray(tmp.T), out_h).T)


def paste_statement(rois, planes, H, W, cls=None):
    """rois [R, >=5] float32, planes [R, h, w] float32 -> float32 [R, H, W]: rule c with the paste.  What leaves the plane is dropped;
    an empty window, a non-finite coordinate or cls < 0 gives an empty mask."""
    R = rois.shape[0]
    out = np.zeros((R, H, W), dtype=np.float32)
    for r in range(R):
        if cls is not None and cls[r] < 0:
            continue
        if not np.all(np.abs(rois[r, 1:5]) < 5e8):
            continue
        x1, y1, x2, y2 = (int(v) for v in rois[r, 1:5])
        roi_w, roi_h = x2 - x1 + 1, y2 - y1 + 1
        if roi_w <= 0 or roi_h <= 0:
            continue
        m = resize_plane(planes[r], roi_w, roi_h)
        ya, yb, xa, xb = max(y1, 0), min(y1 + roi_h, H), max(x1, 0), min(x1 + roi_w, W)
        if ya < yb and xa < xb:
            out[r, ya:yb, xa:xb] = m[ya - y1:yb - y1, xa - x1:xb - x1]
    return out


def pack_statement(masks, threshold):
    """float [R, H, W] -> uint32 [R, H, ceil(W/32)]: bit (c % 32) of word c // 32 = (value >= threshold); bits past W are zero"""
    R, H, W = masks.shape
    Wd = (W + 31) // 32
    bits = np.zeros((R, H, Wd * 32), dtype=np.uint64)
    bits[:, :, :W] = masks >= threshold
    return (bits.reshape(R, H, Wd, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def own_planes(heat, rois):
    return np.ascontiguousarray(heat[np.arange(rois.shape[0]), rois[:, 6].astype(np.int64)])


SIZES = (1, 2, 13, 27, 28, 29, 56, 200, 1344)


@pytest.mark.parametrize("out_h", SIZES)
def test_resize_statement_is_pillows_float_resize(out_h):
    from PIL import Image
    assert int(Image.__version__.split(".")[0]) >= 7, "Pillow < 7 resizes with NEAREST by default"
    rng = np.random.RandomState(100 + out_h)
    for out_w in SIZES:
        p = rng.randn(28, 28).astype(np.float32)
        want = np.array(Image.fromarray(p).resize((out_w, out_h)))
        got = resize_plane(p, out_w, out_h)
        assert want.dtype == np.float32 and got.shape == want.shape == (out_h, out_w)
        assert np.array_equal(got, want), (out_w, out_h, np.abs(got - want).max())


def test_resize_statement_other_plane_sizes():
    """planes that are not 28 x 28 (the golden predict case has 14 x 14), sigmoid-like values in (0, 1)"""
    from PIL import Image
    rng = np.random.RandomState(7)
    for ph, pw, out_w, out_h in ((14, 14, 33, 9), (14, 14, 14, 41), (32, 32, 5, 77), (7, 20, 90, 3), (28, 28, 37, 19), (28, 28, 64, 127)):
        p = rng.rand(ph, pw).astype(np.float32)
        assert np.array_equal(resize_plane(p, out_w, out_h), np.array(Image.fromarray(p).resize((out_w, out_h)))), (ph, pw, out_w, out_h)


def test_paste_statement_reproduces_reference_predict_masks():
    gold = np.load(os.path.join(GOLDEN, "mask_targets_ref.npz"))["predict_masks"]
    rois, heat, info = mcases.predict_case()
    H, W = int(info[0][0]), int(info[0][1])
    assert np.array_equal(paste_statement(rois, own_planes(heat, rois), H, W), gold)
    g = np.load(os.path.join(GOLDEN, "predict_masks_sweep.npz"))
    rois, heat, info, want = g["rois"], g["heatmap"], g["image_info"], g["masks"]
    assert want.shape == (rois.shape[0], 96, 160) and rois.shape[0] >= 24
    got = paste_statement(rois, own_planes(heat, rois), 96, 160)
    for r in range(rois.shape[0]):
        assert np.array_equal(got[r], want[r]), (r, rois[r])


def test_paste_statement_drops_what_leaves_the_plane():
    rng = np.random.RandomState(3)
    planes = rng.rand(5, 28, 28).astype(np.float32)
    rois = np.array([[0, -10, -5, 30, 20], [0, 50, 30, 80, 60], [0, 10, 10, 5, 20], [0, 70, 50, 200, 90], [0, 3, 3, 9, 9]], dtype=np.float32)
    out = paste_statement(rois, planes, 40, 64, cls=np.array([1, 1, 1, 1, -1]))
    assert np.array_equal(out[0, :21, :31], resize_plane(planes[0], 41, 26)[5:, 10:]) and not out[0, 21:].any() and not out[0, :, 31:].any()
    assert np.array_equal(out[1, 30:, 50:], resize_plane(planes[1], 31, 31)[:10, :14])
    assert not out[2].any() and not out[3].any() and not out[4].any()       # empty window, wholly outside, padding row


@pytest.mark.parametrize("W", [160, 77, 32, 5])
def test_pack_statement(W):
    rng = np.random.RandomState(W)
    m = rng.rand(3, 9, W).astype(np.float32)
    m[0, 0, :3] = 0.5                                  # exactly the threshold: set
    m[1, 2, W - 1] = np.nan                            # NaN >= t is false
    words = pack_statement(m, 0.5)
    assert words.dtype == np.uint32 and words.shape == (3, 9, (W + 31) // 32)
    for r in range(3):
        for y in range(9):
            for c in range(words.shape[2] * 32):
                bit = (int(words[r, y, c // 32]) >> (c % 32)) & 1
                assert bit == (1 if c < W and m[r, y, c] >= 0.5 else 0), (r, y, c)
    g = np.load(os.path.join(GOLDEN, "predict_masks_sweep.npz"))["masks"]
    w2 = pack_statement(g, 0.25)
    back = ((w2[:, :, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(g.shape[0], g.shape[1], -1)[:, :, :g.shape[2]].astype(bool)
    assert np.array_equal(back, g >= 0.25)


def test_mask_rows_unpacks_the_packed_statement():
    """scda_amd.infer.mask_rows on host copies: the inverse of the packing, real rows only"""
    import torch
    from scda_amd import infer
    rng = np.random.RandomState(5)
    m = rng.rand(2 * 3, 6, 70).astype(np.float32)
    words = torch.from_numpy(pack_statement(m, 0.5).view(np.int32)).view(2, 3, 6, 3)
    got = infer.mask_rows(words, torch.tensor([2, 0], dtype=torch.int32), 70)
    assert len(got) == 2 and got[0].dtype == np.bool_ and got[0].shape == (2, 6, 70) and got[1].shape == (0, 6, 70)
    assert np.array_equal(got[0], m[:2] >= 0.5)
