"""The rule of the device resize to the original image size (scda_amd/csrc/mask_rescale.hip, include/scda_ops.h), restated in numpy by
tests/mask_orig_np.py, is PIL.Image.resize bit for bit and reproduces tests/golden/segm_orig_ref.npz: the reference's predict_masks,
lines 422-423 of its write_results_to_file and its maskApi.c (tests/golden/make_golden_segm_orig.py).  CPU only; tests/test_mask_orig_gpu.py
compares the kernel with these statements."""
import os

import numpy as np
import pytest

import mask_orig_np as O
import mask_rle_np as RLE
from test_mask_infer_rules import own_planes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_CASES = 8
H, W = 96, 160


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "segm_orig_ref.npz"))


@pytest.fixture(scope="module")
def stated(gold):
    """per case: (sizes, recorded RoI indices, the numpy statement's O [24, oh, ow], its footprints) -- computed once, left unchanged"""
    rois, planes = gold["rois"], own_planes(gold["heatmap"], gold["rois"])
    res = []
    for k in range(N_CASES):
        h, w, oh, ow = (int(v) for v in gold["sizes_%d" % k])
        info = np.array([[h, w, 1.0, oh, ow]], dtype=np.float32)
        out, foot, status = O.statement(rois, planes, H, W, info, rois.shape[0], oh, ow, flag_limits=False)
        assert status[0] == 0
        res.append(((h, w, oh, ow), gold["rois_%d" % k], out, foot))
    return res


def test_fixture_holds_the_cases_of_the_issue(gold):
    sizes = [tuple(int(v) for v in gold["sizes_%d" % k]) for k in range(N_CASES)]
    assert sizes == [(96, 160, 60, 100), (96, 160, 24, 40), (96, 160, 137, 229), (96, 160, 96, 160), (96, 160, 48, 160),
                     (96, 160, 96, 100), (96, 160, 1, 1), (90, 150, 54, 90)]
    assert gold["rois"].shape == (24, 7) and int(str(gold["pillow"]).split(".")[0]) >= 7
    for k in range(N_CASES - 1):
        assert np.array_equal(gold["rois_%d" % k], np.arange(24))
    assert 8 <= len(gold["rois_7"]) < 24                       # the reference raises for a RoI that leaves the 90 x 150 image
    assert os.path.getsize(os.path.join(GOLDEN, "segm_orig_ref.npz")) < 1 << 20


@pytest.mark.parametrize("k", range(N_CASES))
def test_statement_reproduces_the_reference(gold, stated, k):
    (h, w, oh, ow), idx, out, _ = stated[k]
    want = gold["orig_%d" % k]
    strings = gold["rle_%d" % k].tobytes().split(b"\n")
    assert want.shape == (len(idx), oh, ow) and len(strings) == len(idx)
    for i, r in enumerate(idx):
        assert np.array_equal(out[r], want[i]), (k, r)
        assert not np.signbit(out[r][out[r] == 0]).any()       # no negative zeros: the outside is +0.0f
        assert RLE.to_string(RLE.encode(out[r] > 0.5)) == strings[i], (k, r)


@pytest.mark.parametrize("k", range(N_CASES))
def test_statement_is_pillows_resize_of_the_sub_plane(gold, stated, k):
    """also for the RoIs the fixture cannot hold: P is the h x w sub-plane, so Pillow clamps at w, not at the padded W"""
    from PIL import Image
    (h, w, oh, ow), _, out, _ = stated[k]
    rois, planes = gold["rois"], own_planes(gold["heatmap"], gold["rois"])
    for r in range(rois.shape[0]):
        P = O.sub_plane(rois[r], planes[r], H, W, h, w)
        assert P.shape == (h, w)
        assert np.array_equal(out[r], np.array(Image.fromarray(P).resize((ow, oh)))), (k, r)


def test_equal_sizes_give_the_pasted_plane(gold, stated):
    masks = np.load(os.path.join(GOLDEN, "predict_masks_sweep.npz"))["masks"]
    assert np.array_equal(stated[3][2], masks)


def test_wrong_clamp_would_show(gold, stated):
    """the (90, 150) case differs from resizing the padded 96 x 160 plane cropped afterwards -- the case can tell the two apart"""
    from PIL import Image
    rois, planes = gold["rois"], own_planes(gold["heatmap"], gold["rois"])
    r = 3                                                        # the whole image
    padded = O.sub_plane(rois[r], planes[r], H, W, H, W)
    wrong = np.array(Image.fromarray(padded).resize((96, 58)))[:54, :90]
    assert not np.array_equal(stated[7][2][r], wrong)


@pytest.mark.parametrize("k", range(N_CASES))
def test_nothing_outside_the_footprint(stated, k):
    _, _, out, foot = stated[k]
    for r in range(out.shape[0]):
        fx1, fy1, fx2, fy2 = (int(v) for v in foot[r, 1:])
        inside = np.zeros(out[r].shape, dtype=bool)
        inside[fy1:fy2 + 1, fx1:fx2 + 1] = True
        assert not out[r][~inside].any(), (k, r)
        assert k == 7 or (fx2 >= fx1 and fy2 >= fy1)             # on the 96 x 160 image every RoI of the sweep has a window


def test_footprint_is_tight_on_identity_and_empty_for_padding(gold):
    roi = np.array([0, 10, 20, 30, 40], dtype=np.float32)
    assert O.footprint(roi, 96, 160, 96, 160) == (10, 20, 30, 40)
    assert O.footprint(roi, 96, 160, 96, 160, cls=-1) == (0, 0, -1, -1)
    assert O.footprint(np.array([0, 200, 20, 230, 40], dtype=np.float32), 96, 160, 60, 100) == (0, 0, -1, -1)
    fx1, fy1, fx2, fy2 = O.footprint(roi, 96, 160, 48, 80)       # 2x down: support 4 input samples
    assert (fx1, fx2, fy1, fy2) == (3, 16, 8, 21)              # X = 17: xmin = int(35 - 4 + 0.5) = 31, past the window


def test_pack_gt_is_strictly_greater_and_clears_outside():
    v = np.zeros((1, 3, 40), dtype=np.float32)
    v[0, 0, :5] = 0.5
    v[0, 1, 33] = 0.75
    v[0, 2, :] = 1.0                                             # row 2 lies outside oh = 2
    v[0, 0, 39] = 1.0                                            # column 39 lies outside ow = 38
    words = O.pack_gt(v, 0.5, [(2, 38)])
    assert words.shape == (1, 3, 2) and not words[0, 0].any() and not words[0, 2].any()
    assert words[0, 1, 0] == 0 and words[0, 1, 1] == 2
    low = O.pack_gt(v, -0.1, [(2, 38)])                          # a negative threshold sets the outside of the window, inside oh x ow
    assert low[0, 0, 0] == 0xffffffff and low[0, 0, 1] == 0x3f and not low[0, 2].any()


def test_limits():
    assert O.status_of([96, 160, 1, 60, 100], 96, 160, 64, 128) == 0
    assert O.status_of([96, 160, 1, 24, 40], 96, 160, 64, 128) == 0                  # 4x down: the limit itself
    assert O.status_of([96, 160, 1, 23, 40], 96, 160, 64, 128) == O.FLAG_RATIO
    assert O.status_of([96, 160, 1, 65, 100], 96, 160, 64, 128) == O.FLAG_CAPACITY
    assert O.status_of([96, 160, 1, 0, 100], 96, 160, 64, 128) == O.FLAG_EMPTY | O.FLAG_RATIO
    assert O.status_of([97, 160, 1, 60, 100], 96, 160, 64, 128) == O.FLAG_INPUT
    assert O.status_of([96, 160, 1, float("nan"), 100], 96, 160, 64, 128) == O.FLAG_INPUT
    assert O.status_of([96, 160, 1, 1, 1], 96, 160, 64, 128) == O.FLAG_RATIO
