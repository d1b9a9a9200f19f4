"""The heat-map decode on the MI355X at its structural edges (scda_amd/csrc/keypoint_ops.hip): native.keypoint_decode against the host
rule (dropin.functions.mask.predict_keypoints: PIL's resize + np.argmax), the bits of all three columns.  tests/test_keypoint_gpu.py
decodes random planes, which never tie; here are image sizes on the partition edges (128-column strips, 64-row refills), exact ties
across both kinds of boundary -- each test first shows on the host that the tie it means to create exists --, the row-major order
against the strip order, one-column and one-row slivers, the layouts the head hands over and the refusals."""
import numpy as np
import pytest
import torch

from gpu_arrays import bits as _bits, dev as _dev

pytestmark = pytest.mark.gpu

STRIP, REFILL = 128, 64                                                 # keypoint_ops.hip: kStrip, kRows


def _decode(cuda, rois, heat, H, W, src=None, cls=None):
    """-> the host rule's rows, after the kernel's were found equal to them bit for bit"""
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_keypoints
    rois = np.asarray(rois, dtype=np.float32)
    want = predict_keypoints(rois, heat, np.array([[H, W, 1.0]], dtype=np.float32), cls=cls)
    got = N.keypoint_decode(_dev(rois, cuda), _dev(heat, cuda) if src is None else src, H, W,
                            cls=None if cls is None else _dev(cls, cuda)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want)), (H, W, rois.tolist(), got.tolist(), want.tolist())
    return want


def _randn(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


@pytest.mark.parametrize("H,W", [(70, w) for w in (1, 127, 128, 129, 256, 257)] + [(h, 130) for h in (1, 63, 64, 65, 129)])
def test_image_sizes_on_the_partition_edges(cuda, H, W):
    """one RoI that is the image, one that hangs over every side; random 56 x 56 planes"""
    rois = [[0, 0, 0, W - 1, H - 1], [0, -5, -4, W + 3, H + 6]]
    want = _decode(cuda, rois, _randn(H * 1000 + W, 2, 2, 56, 56), H, W)
    assert (want[..., 0] < W).all() and (want[..., 1] < H).all() and want[..., 2].all()


# ------------------------------------------------------------------------------------------------------------------- ties
TIE_H, TIE_W = 140, 300                                                 # three strips (128 + 128 + 44), three refills (64 + 64 + 12)
TIE_ROIS = [[0, 0, 0, TIE_W - 1, TIE_H - 1], [0, -40, -30, TIE_W - 1, TIE_H - 1]]      # the image; clipped on the left and at the top


def _tie_planes():
    col = np.repeat(_randn(5, 1, 56), 56, 0)                            # every row the same: the resized rows are identical
    row = np.repeat(_randn(6, 56, 1), 56, 1)                            # every column the same
    const = lambda v: np.full((56, 56), v, dtype=np.float32)            # noqa: E731
    return {"zero": const(0.0), "one": const(1.0), "minus_2.7": const(-2.7), "nan": const(np.nan), "minus_inf": const(-np.inf),
            "plus_inf": const(np.inf), "column_constant": col, "row_constant": row}


def _winners(seen):
    """np.argmax's candidates: the NaNs when there is one, else the places of the maximum"""
    nan = np.isnan(seen)
    return nan if nan.any() else seen == seen.max()


def _visible(plane, roi, H, W):
    """the host's view of one window: (the resized plane's visible part, image x of its first column, image y of its first row)"""
    from PIL import Image
    x1, y1, x2, y2 = (int(v) for v in roi[1:5])
    full = np.array(Image.fromarray(plane).resize((x2 - x1 + 1, y2 - y1 + 1)))
    xa, xb, ya, yb = max(x1, 0), min(x2 + 1, W), max(y1, 0), min(y2 + 1, H)
    return full[ya - y1:yb - y1, xa - x1:xb - x1], xa, ya


@pytest.mark.parametrize("name", sorted(_tie_planes()))
def test_ties_across_strips_and_refills(cuda, name):
    """planes whose resized window attains its maximum in many places: np.argmax's winner is the first of them in row-major order of
    the visible part, whichever strip or refill holds it"""
    plane = _tie_planes()[name]
    across_strips = across_refills = False
    for roi in TIE_ROIS:
        seen, xa, ya = _visible(plane, roi, TIE_H, TIE_W)
        hit = _winners(seen)
        cols, rows = np.nonzero(hit.any(0))[0] + xa, np.nonzero(hit.any(1))[0]      # image columns; rows counted from the first visible
        strips, refills = set((cols // STRIP).tolist()), set((rows // REFILL).tolist())
        if name != "column_constant":                                   # (its maximum is one column, in every row)
            assert strips == {0, 1, 2}, (name, roi, sorted(strips))
            across_strips = True
        if name != "row_constant":
            assert refills == {0, 1, 2}, (name, roi, sorted(refills))
            across_refills = True
        assert hit.sum() >= 3
    assert across_strips or across_refills
    heat = np.stack([plane[None], plane[None]])                         # R = 2, Kp = 1
    want = _decode(cuda, TIE_ROIS, heat, TIE_H, TIE_W)
    for r, roi in enumerate(TIE_ROIS):                                  # and the host's winner is the first candidate
        seen, xa, ya = _visible(plane, roi, TIE_H, TIE_W)
        py, px = np.unravel_index(np.argmax(_winners(seen)), seen.shape)
        assert tuple(want[r, 0, :2]) == (xa + px, ya + py)
        if name not in ("column_constant", "row_constant"):
            assert (px, py) == (0, 0)                                   # the first visible pixel


@pytest.mark.parametrize("nan", [False, True])
def test_the_earlier_row_wins_from_the_later_strip(cuda, nan):
    """a 64 x 64 plane pasted at identity size at x1 = 96: the same maximum at plane (3, 40) -- image column 136, strip 1 -- and at
    plane (5, 2) -- column 98, strip 0; row 3 comes first in row-major order.  Then two NaNs there under a larger finite value"""
    H, W, x1, y1 = 80, 200, 96, 7
    plane = _randn(21, 64, 64)
    plane[10, 10] = 50.0 if nan else 3.0
    plane[3, 40] = plane[5, 2] = np.nan if nan else 9.0
    roi = [0, x1, y1, x1 + 63, y1 + 63]
    seen, xa, ya = _visible(plane, roi, H, W)
    assert np.array_equal(_bits(seen), _bits(plane)) and (x1 + 40) // STRIP == 1 and (x1 + 2) // STRIP == 0     # identity: a copy
    want = _decode(cuda, [roi], plane[None, None], H, W)
    assert tuple(want[0, 0, :2]) == (x1 + 40, y1 + 3) and (np.isnan(want[0, 0, 2]) if nan else want[0, 0, 2] == 9.0)


# ---------------------------------------------------------------------------------------------------------------- slivers
def test_one_visible_column_or_row(cuda):
    H, W = 70, 200
    rois = [[0, W - 1, 10, W + 29, 40],       # only image column W - 1, the window's first
            [0, 100, 5, 128, 50],             # strip 1 sees one column of it: 128, its first
            [0, 128, 5, 160, 50],             # starts on a strip's first column
            [0, -30, 5, 0, 40]]               # only the window's LAST column, at image column 0
    heat = _randn(31, 4, 2, 56, 56)
    want = _decode(cuda, rois, heat, H, W)
    assert (want[0, :, 0] == W - 1).all() and (want[3, :, 0] == 0).all()
    # the same with the best value of window 1 forced into its last column: the one-column strip holds the winner
    heat[1, :, :, 55] += 100.0
    want = _decode(cuda, rois, heat, H, W)
    assert (want[1, :, 0] == 128).all()
    rois = [[0, 10, H - 1, 50, H + 20], [0, 10, -20, 50, 0], [0, 120, -20, 135, 0], [0, 7, 9, 7, 9]]     # one row; 56 -> 1 on both axes
    want = _decode(cuda, rois, _randn(32, 4, 2, 56, 56), H, W)
    assert (want[0, :, 1] == H - 1).all() and (want[1, :, 1] == 0).all() and (want[2, :, 1] == 0).all()
    assert (want[3, :, :2] == (7, 9)).all()


@pytest.mark.parametrize("h", [1, 2, 21, 22])
def test_rows_of_a_64_row_plane_scaled_down(cuda, h):
    """64 -> 1, 2, 21, 22 rows: either side of where the vertical table stops holding a run's weights (keypoint_ops.hip: 64 rows
    down-scaled to more than 21), on an up-scaled and on a down-scaled horizontal axis"""
    H, W = 70, 203
    rois = [[0, 10, 3, 40, 3 + h - 1], [0, 90, 30, 190, 30 + h - 1], [0, 120, H - h + 1, 135, H]]
    _decode(cuda, rois, _randn(40 + h, 3, 2, 64, 64), H, W)


# ---------------------------------------------------------------------------------------------------------------- layouts
def test_layouts(cuda):
    H, W = 70, 203
    rois = np.array([[0, -10, -5, 30, 20], [0, 100, 7, 202, 69], [0, 120, 60, 140, 80]], dtype=np.float32)
    heat = _randn(50, 3, 17, 56, 56)                                    # Kp = 17
    _decode(cuda, rois, heat, H, W)
    tall = _dev(heat.transpose(1, 0, 2, 3), cuda).view(17, 3, 56, 56).transpose(0, 1)       # the channel-major head's view
    assert not tall.is_contiguous()
    _decode(cuda, rois, heat, H, W, src=tall)
    one = _dev(heat[:1], cuda).expand(3, 17, 56, 56)                    # stride 0 over the RoIs: every RoI decodes the same maps
    assert one.stride(0) == 0
    _decode(cuda, rois, np.repeat(heat[:1], 3, 0), H, W, src=one)


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(cuda):
    from scda_amd import native as N
    rois = _dev(np.array([[0, 0, 0, 9, 9]], dtype=np.float32), cuda)
    heat = _dev(_randn(60, 1, 1, 56, 56), cuda)
    out = torch.full((1, 1, 3), -7.0, device=cuda)
    ws = torch.empty(4096, dtype=torch.uint8, device=cuda)
    side = 46341                                                        # 46341^2 >= 2^31: positions y * W + x no longer fit an int
    assert side * side >= 2 ** 31 > (side - 1) * (side - 1)
    st = N.lib().scda_keypoint_decode_hip(rois.data_ptr(), 5, None, heat.data_ptr(), 56 * 56, 56 * 56, 56, 1, 1, 1, 56, 56, side, side,
                                          ws.data_ptr(), out.data_ptr(), None)
    assert st != 0
    with pytest.raises(N.ScdaNativeError):
        N.keypoint_decode(rois, heat, side, side, out=out)
    need = N.keypoint_decode_workspace_bytes(1, 1, 300)
    assert need > 0
    with pytest.raises(ValueError, match="ws"):                         # one byte short, through the wrapper
        N.keypoint_decode(rois, heat, 140, 300, out=out, ws=torch.empty(need - 1, dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    N.keypoint_decode(rois, heat, 140, 300, out=out, ws=torch.empty(need, dtype=torch.uint8, device=cuda))     # and enough is enough
    assert (out.cpu().numpy()[0, 0, :2] < 10).all()
