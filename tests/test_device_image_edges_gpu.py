"""The device data path at its structural edges (scda_amd/csrc/image_ops.hip): one- and two-pixel sides on either end, extreme
down-scales (a window of 1201 taps for 300 -> 1), saturated input under the filter with the largest negative lobes, a row band with
row0 > 0 -- the `- row0` arithmetic of the vertical pass, which device_image.resize_tables never exercises -- and the refusals.
Everything against PIL (Image.resize [+ FLIP_LEFT_RIGHT] + data.to_tensor + data.normalize) with torch.equal; the host tables equal
PIL's at all these sizes (tests/test_device_image.py), so PIL alone is the reference for the kernels."""
import numpy as np
import pytest
import torch

from test_device_image import EDGE_SIZES, PIL_FILTERS

pytestmark = pytest.mark.gpu


def _cpu_path(a, new_w, new_h, flip, do_norm, filter="bicubic"):
    from PIL import Image
    from scda_amd import data as D
    img = Image.fromarray(a if a.shape[-1] != 1 else a[:, :, 0]).resize((new_w, new_h), PIL_FILTERS[filter])
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    t = D.to_tensor(img)
    return D.normalize(t) if do_norm else t


def _image(H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


@pytest.mark.parametrize("H,W,nh,nw", EDGE_SIZES)
@pytest.mark.parametrize("C", [1, 3])
def test_degenerate_sizes_equal_pil(cuda, H, W, nh, nw, C):
    from scda_amd import device_image as DI
    a = _image(H, W, C, H * 7 + W + C)
    for flip in (False, True):
        for norm in (True, False):
            got = DI.resize_to_tensor(a, nw, nh, cuda, normalize=norm, flip=flip)
            ref = _cpu_path(a, nw, nh, flip, norm)
            assert got.shape == ref.shape == (C, nh, nw) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), ref), (flip, norm)


@pytest.mark.parametrize("H,W,nh,nw", [(300, 400, 1, 1), (64, 64, 63, 65)])
@pytest.mark.parametrize("filter", ["box", "lanczos"])
def test_other_filters_at_the_extremes(cuda, H, W, nh, nw, filter):
    from scda_amd import device_image as DI
    for C in (1, 3):
        a = _image(H, W, C, 11 + C)
        got = DI.resize_to_tensor(a, nw, nh, cuda, filter=filter)
        assert torch.equal(got.cpu(), _cpu_path(a, nw, nh, False, True, filter)), C


def test_saturated_input_under_lanczos(cuda):
    """all 255 and a 0 / 255 checkerboard, 300 x 400 -> 7 x 5 with lanczos: the largest negative lobes against the int32 sums"""
    from scda_amd import device_image as DI
    full = np.full((300, 400, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:300, 0:400]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    blocks = np.repeat((((yy // 43 + xx // 80) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)       # squares about a window wide
    for a in (full, board, blocks):
        for norm in (False, True):
            got = DI.resize_to_tensor(a, 5, 7, cuda, normalize=norm, filter="lanczos")
            assert torch.equal(got.cpu(), _cpu_path(a, 5, 7, False, norm, "lanczos"))


def _band_tables(W, out_w, row0, rows, out_h, cuda):
    """tables for resizing rows [row0, row0 + rows) of an image: the vertical axis is the band's own, its first samples counted in
    image rows (the ABI: bounds_v are image rows, the kernel subtracts row0)"""
    from scda_amd import device_image as DI
    from scda_amd import native as N
    bh, kh, ksh = DI.axis_coeffs(W, out_w)
    bv, kv, ksv = DI.axis_coeffs(rows, out_h)
    bv = bv.copy()
    bv[:, 0] += row0
    assert bv[:, 0].min() >= row0 and (bv[:, 0] + bv[:, 1]).max() <= row0 + rows         # correct tables only: the kernel trusts them
    assert bh[:, 0].min() >= 0 and (bh[:, 0] + bh[:, 1]).max() <= W
    return (N.upload(bh, cuda), N.upload(kh, cuda), ksh, N.upload(bv, cuda), N.upload(kv, cuda), ksv, row0, rows)


@pytest.mark.parametrize("row0", [1, 13])
@pytest.mark.parametrize("rows", [1, 27])
def test_a_row_band_equals_pil_on_the_crop(cuda, row0, rows):
    from PIL import Image
    from scda_amd import data as D
    from scda_amd import native as N
    H, W = 40, 52
    for C, (out_h, out_w) in ((3, (11, 31)), (1, (rows, 70)), (3, (33, 52))):      # down, identity (a skipped pass), up
        a = _image(H, W, C, 100 + row0 + rows + C)
        img = Image.fromarray(a if C == 3 else a[:, :, 0])
        ref = D.normalize(D.to_tensor(img.crop((0, row0, W, row0 + rows)).resize((out_w, out_h))))
        got = N.image_resize_normalize(N.upload(a, cuda), _band_tables(W, out_w, row0, rows, out_h, cuda), out_h, out_w)
        assert torch.equal(got.cpu(), ref), (C, out_h, out_w)


def test_refusals_launch_nothing(cuda):
    from scda_amd import device_image as DI
    from scda_amd import native as N
    H, W, C, oh, ow = 40, 52, 3, 11, 31
    src = N.upload(_image(H, W, C, 5), cuda)
    bh, kh, ksh, bv, kv, ksv, row0, rows = DI.resize_tables(H, W, oh, ow, cuda)
    assert (row0, rows) == (0, H)
    out = torch.full((C, oh, ow), -7.0, device=cuda)
    nb = int(N.lib().scda_image_resize_tmp_bytes(rows, ow, C))
    assert nb == rows * ow * C
    tmp = torch.full((nb,), 77, dtype=torch.uint8, device=cuda)

    def call(row0=row0, rows=rows, tmp_bytes=nb, normalize=1, std=0.5):
        return N.lib().scda_image_resize_normalize_hip(N._p(src), H, W, C, N._p(bh), N._p(kh), ksh, ow, N._p(bv), N._p(kv), ksv, oh, row0, rows,
                                                       N._p(tmp), tmp_bytes, normalize, 0.5, std, 0, N._p(out), N._stream())
    for kw in (dict(row0=1), dict(row0=-1), dict(rows=H + 1), dict(rows=0), dict(row0=H, rows=1),      # a band outside the image
               dict(tmp_bytes=nb - 1), dict(std=0.0)):
        assert call(**kw) == -1, kw                                     # SCDA_EINVAL
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (tmp == 77).all()
    assert call(normalize=0, std=0.0) == 0                              # std plays no part without Normalize
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, DI.resize_to_tensor(src.cpu().numpy(), ow, oh, cuda))
