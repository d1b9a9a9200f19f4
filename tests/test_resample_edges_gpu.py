"""The edges of the shared windowed resampler (scda_amd/csrc/mask_resample.h) through its three consumers: ONE table of RoI windows
goes through the paste (mask_ops.hip), the resize to the original size (mask_rescale.hip) and the keypoint decode (keypoint_ops.hip).
Expected values come from the statements the project has pinned to the reference -- paste_statement / pack_statement
(tests/test_mask_infer_rules.py), mask_orig_np.statement / pack_gt and dropin.functions.mask.predict_keypoints -- and every comparison
is equality of the uint32 views.  The CPU test at the end keeps those statements equal to PIL on the very sizes of the table."""
import functools

import numpy as np
import pytest
import torch

import mask_orig_np as O
from gpu_arrays import bits, dev, words
from test_mask_infer_rules import pack_statement, paste_statement, resize_plane

# two 128-column strips, the second partly used; W no multiple of 32 or of 4; two 64-row refills
H, W = 70, 150
MASK_SIDES, KEYPOINT_SIDES = (14, 28), (56, 64)
NAN = float('nan')


def windows(ph, pw):
    """(x1, y1, x2, y2) of the table for planes of ph x pw; the last entry of a row says whether anything of it is visible"""
    table = [
        (120, 3, 140, 20, True),                    # straddles column 128
        (100, 5, 127, 30, True),                    # ends at column 127
        (128, 5, 149, 30, True),                    # starts at column 128
        (10, 60, 40, 69, True),                     # crosses row 64
        (0, 0, 149, 69, True),                      # the whole image
        (7, 9, 7 + pw - 1, 9 + ph - 1, True),       # identity on both axes
        (7, 9, 7 + pw - 1, 21, True),               # identity on x only
        (90, 1, 102, 1 + ph - 1, True),             # identity on y only
        (20, 2, 24, 61, True),                      # roi_w = 5 (down), roi_h = 60
        (2, 20, 61, 24, True),                      # its transpose
        (33, 44, 33, 44, True),                     # 1 x 1
        (-10, -5, 30, 20, True),                    # partly left / top of the image
        (130, 50, 170, 90, True),                   # partly right / bottom of the image
        (200, 10, 230, 30, False),                  # wholly outside
        (50, 10, 40, 30, False),                    # x2 < x1
        (NAN, 0, 5, 5, False),                      # a non-finite coordinate
        (0, 0, 6e8, 5, False),                      # a coordinate beyond the int range the kernels accept
        (100, 7, 131.9, 34.2, True),                # fractional coordinates
        (3, 3, 30, 30, False),                      # the padding slot (cls = -1 below)
    ]
    rois = np.array([(0,) + t[:4] for t in table], dtype=np.float32)
    cls = np.ones(len(table), dtype=np.int32)
    cls[-1] = -1
    return rois, cls, np.array([t[4] for t in table])


def sizes_in_table():
    """every (plane side, roi_w, roi_h) of a window the kernels resize"""
    out = set()
    for side in MASK_SIDES + (32,) + KEYPOINT_SIDES:
        rois, _, _ = windows(side, side)
        for x1, y1, x2, y2 in rois[:, 1:5]:
            if np.all(np.abs([x1, y1, x2, y2]) < 5e8) and int(x2) >= int(x1) and int(y2) >= int(y1):
                out.add((side, int(x2) - int(x1) + 1, int(y2) - int(y1) + 1))
    return sorted(out)


def planes_of(side, seed, lead=()):
    return np.random.RandomState(seed).rand(len(windows(side, side)[0]), *lead, side, side).astype(np.float32)


@functools.lru_cache(maxsize=None)
def paste_case(side):
    """(rois, cls, visible, planes, statement with cls, statement without): computed once, left unchanged"""
    rois, cls, visible = windows(side, side)
    planes = planes_of(side, 100 + side)
    return rois, cls, visible, planes, paste_statement(rois, planes, H, W, cls), paste_statement(rois, planes, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("side", MASK_SIDES + (32,))
def test_paste_float_and_packed(cuda, side):
    from scda_amd import native as N
    rois, cls, visible, planes, want_cls, want_all = paste_case(side)
    assert all(want_cls[i].any() == visible[i] for i in range(len(visible))) and want_all[-1].any()
    for c, want in ((cls, want_cls), (None, want_all)):
        dc = None if c is None else dev(c, cuda)
        out = torch.full((rois.shape[0], H, W), 777.0, device=cuda)
        N.mask_paste(dev(rois, cuda), dev(planes, cuda), H, W, cls=dc, out=out)
        assert np.array_equal(words(out), bits(want))                 # every element written, no negative zero
        for threshold in (0.5, 0.0, -0.1):
            got = N.mask_paste(dev(rois, cuda), dev(planes, cuda), H, W, cls=dc, packed=True, threshold=threshold)
            assert np.array_equal(words(got), pack_statement(want, threshold)), threshold


# per image (h, w) = (70, 150); the original sizes: up-scale, identity, down-scale by 2, just inside the ratio limit of 4, over it
ORIGINALS = ((93, 201), (70, 150), (35, 75), (18, 38), (17, 38))
HO, WO = 93, 201


@functools.lru_cache(maxsize=None)
def rescale_case(side, with_cls):
    rois, cls, _ = windows(side, side)
    n = rois.shape[0]
    planes = planes_of(side, 200 + side)
    B = len(ORIGINALS)
    info = np.array([[H, W, 1.0, oh, ow] for oh, ow in ORIGINALS], dtype=np.float32)
    all_rois = np.concatenate([rois] * B)
    all_rois[:, 0] = np.repeat(np.arange(B), n)
    all_planes, all_cls = np.concatenate([planes] * B), np.concatenate([cls] * B)
    want, foot, status = O.statement(all_rois, all_planes, H, W, info, n, HO, WO, cls=all_cls if with_cls else None)
    sizes = [(oh, ow) if status[b] == 0 else (0, 0) for b, (oh, ow) in enumerate(ORIGINALS) for _ in range(n)]
    return all_rois, all_planes, all_cls, info, want, foot, status, sizes


@pytest.mark.gpu
@pytest.mark.parametrize("side,with_cls", [(14, True), (28, True), (28, False), (32, True)])
def test_rescale_float_and_packed(cuda, side, with_cls):
    from scda_amd import native as N
    rois, planes, cls, info, want, foot, status, sizes = rescale_case(side, with_cls)
    n = rois.shape[0] // len(ORIGINALS)
    assert list(status) == [0, 0, 0, 0, O.FLAG_RATIO] and not want[4 * n:].any() and all(want[b * n].any() for b in range(4))
    args = (dev(rois, cuda), dev(planes, cuda), H, W, dev(info, cuda), HO, WO)
    dc = dev(cls, cuda) if with_cls else None
    out = torch.full(want.shape, 777.0, device=cuda)
    _, got_foot, got_status = N.mask_rescale(*args, cls=dc, out=out)
    assert np.array_equal(words(out), bits(want))
    assert np.array_equal(got_status.cpu().numpy(), status) and np.array_equal(got_foot.cpu().numpy(), foot.astype(np.float32))
    for threshold in (0.5, 0.0, -0.1):
        got, got_foot, got_status = N.mask_rescale(*args, cls=dc, packed=True, threshold=threshold)
        assert np.array_equal(words(got), O.pack_gt(want, threshold, sizes)), threshold
        assert np.array_equal(got_status.cpu().numpy(), status) and np.array_equal(got_foot.cpu().numpy(), foot.astype(np.float32))
        assert not words(got)[4 * n:].any()                            # the image over the ratio limit: flagged, its masks empty


@pytest.mark.gpu
@pytest.mark.parametrize("side", KEYPOINT_SIDES)
def test_keypoint_decode(cuda, side):
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_keypoints
    rois, cls, visible = windows(side, side)
    heat = np.random.RandomState(300 + side).randn(rois.shape[0], 2, side, side).astype(np.float32)
    info = np.array([[H, W, 1.0]], dtype=np.float32)
    for c in (cls, None):
        want = predict_keypoints(rois, heat, info, cls=c)
        got = N.keypoint_decode(dev(rois, cuda), dev(heat, cuda), H, W, cls=None if c is None else dev(c, cuda))
        assert np.array_equal(words(got), bits(want)), (got.cpu().numpy(), want)
        assert all(want[i].any() == (visible[i] or (c is None and i == len(visible) - 1)) for i in range(len(visible)))


def test_statements_equal_pil_on_the_tables_sizes():
    """runs without a GPU: what the kernels are compared with above is Pillow's own resize on every (plane side, roi_w, roi_h) of the
    table"""
    from PIL import Image
    assert int(Image.__version__.split(".")[0]) >= 7, "Pillow < 7 resizes with NEAREST by default"
    cases = sizes_in_table()
    assert cases
    for side, roi_w, roi_h in cases:
        p = np.random.RandomState(side * 1000 + roi_w).randn(side, side).astype(np.float32)
        want = np.array(Image.fromarray(p).resize((roi_w, roi_h)))
        assert np.array_equal(bits(resize_plane(p, roi_w, roi_h)), bits(want)), (side, roi_w, roi_h)
