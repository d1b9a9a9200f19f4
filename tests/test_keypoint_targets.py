"""Keypoint targets of the training keypoint branch, host side (no GPU): dropin.functions.mask.compute_keypoint_targets.  The RoI
selection is compute_mask_targets' (pinned to the reference by tests/test_mask_targets.py); the target rule is this project's own
(include/scda_ops.h: the inverse of the keypoint decode) and is checked against a plain-loop restatement, at its edges, and through the
decode itself: a heat map that is 1 at the target decodes to a pixel next to the keypoint."""
import math

import numpy as np
import pytest
import torch

import mask_cases as mcases


@pytest.fixture()
def cpu_backend():
    """the IoU matrix of the host functions on the C oracle (the product computes it on the MI355X)"""
    from oracle import native_ops as orc
    from scda_amd.dropin import backend
    backend.use(bbox_overlaps=lambda b, q: orc.bbox_overlaps(b[:, :4], q[:, :4]),
                nms=lambda d, t: torch.from_numpy(orc.nms(d.numpy(), t)))
    yield
    backend.reset()


def rule(roi, kp, mw, mh):
    """the rule of include/scda_ops.h for one integer RoI and one keypoint, in Python floats (float64)"""
    x1, y1, x2, y2 = (float(int(c)) for c in roi)
    kx, ky, v = (float(c) for c in kp)
    roi_w, roi_h = x2 - x1 + 1.0, y2 - y1 + 1.0
    if not (v > 0 and x1 <= kx < x2 + 1.0 and y1 <= ky < y2 + 1.0):
        return -1
    bx = min(math.floor((kx - x1) * mw / roi_w), mw - 1)
    by = min(math.floor((ky - y1) * mh / roi_h), mh - 1)
    return by * mw + bx


def keypoints_for(gts, Kp, seed):
    """[B, G, Kp, 3] float64: points in and a little around every box, v in {0, 1, 2}; padded (zero) rows get points too"""
    rng = np.random.RandomState(seed)
    B, G = gts.shape[:2]
    x1, y1, x2, y2 = (gts[..., c].astype(np.float64)[..., None] for c in range(4))
    u = rng.uniform(-0.15, 1.15, size=(B, G, Kp, 2))
    kps = np.zeros((B, G, Kp, 3))
    kps[..., 0] = x1 + u[..., 0] * (x2 - x1 + 1)
    kps[..., 1] = y1 + u[..., 1] * (y2 - y1 + 1)
    kps[..., 2] = rng.randint(0, 3, size=(B, G, Kp))
    return kps


def kp_cfg(cfg, mw=56, mh=56):
    return {k: v for k, v in dict(cfg, label_w=mw, label_h=mh).items() if k != 'num_classes'}


@pytest.mark.parametrize("name", list(mcases.CASES))
def test_targets_equal_the_plain_loop_rule(name, cpu_backend):
    from scda_amd.dropin.functions.mask import compute_keypoint_targets
    from scda_amd.dropin.utils import bbox_helper
    props, gts, _, info, cfg = mcases.make(name)
    Kp, (mw, mh) = 7, ((56, 56) if name != "two_images_ragged" else (20, 14))
    kps = keypoints_for(gts, Kp, 3)
    np.random.seed(11)
    rois, targets = compute_keypoint_targets(torch.from_numpy(props), kp_cfg(cfg, mw, mh), torch.from_numpy(gts), kps, torch.from_numpy(info))
    assert rois.dtype == torch.float32 and targets.dtype == torch.int32 and not rois.is_cuda and not targets.is_cuda
    rois, targets = rois.numpy(), targets.numpy()
    if name == "no_positive":                                     # the placeholder of the mask path
        assert rois.shape == (1, 5) and not rois.any() and targets.shape == (1, Kp) and (targets == -1).all()
        return
    assert rois.shape[1] == 5 and targets.shape == (rois.shape[0], Kp) and rois.shape[0] >= 2
    counted = 0
    for r, row in enumerate(rois):
        b = int(row[0])
        keep = np.where(gts[b][:, 2] > gts[b][:, 1] + 1)[0]
        g = keep[bbox_helper.bbox_iou_overlaps(row[None, 1:5], gts[b][keep]).argmax(axis=1)[0]]
        want = [rule(row[1:5], kps[b, g, k], mw, mh) for k in range(Kp)]
        assert targets[r].tolist() == want, (r, row, targets[r], want)
        counted += sum(w >= 0 for w in want)
    assert 0 < counted < targets.size and targets.max() < mw * mh


def test_rule_edges(cpu_backend):
    """through the whole function: ground-truth boxes as the only RoIs (append_gts), a zero-padded row between them"""
    from scda_amd.dropin.functions.mask import compute_keypoint_targets, keypoint_target_bins
    cfg = {'positive_iou_thresh': 0.5, 'batch_size_per_image': 64, 'label_h': 56, 'label_w': 56, 'append_gts': True}
    gts = np.array([[[10, 20, 49, 59, 1], [0, 0, 0, 0, 0], [100, 5, 163, 40, 2]]], dtype=np.float32)
    below = lambda v: float(np.nextafter(np.float64(v), 0.0))       # noqa: E731
    a = [(10, 20, 2),                    # kx == x1, ky == y1: bin (0, 0)
         (below(50), 30, 2),             # just below x2 + 1: the last column
         (50, 30, 2),                    # kx == x2 + 1: outside
         (30, 30, 0),                    # not labelled
         (30, below(60), 1),             # just below y2 + 1: the last row
         (below(10), 30, 2),             # just left of x1
         (30, 60, 2)]                    # ky == y2 + 1
    pad = [(30, 30, 2)] * len(a)         # the padded row's keypoints lie inside box 0: they must never be read
    b = [(100 + 64 * (i + 0.5) / 7, 5 + 36 * (i + 0.5) / 7, 2) for i in range(len(a))]
    kps = np.array([[a, pad, b]], dtype=np.float64)
    info = np.array([[80, 200, 1.0]], dtype=np.float32)
    rois, targets = compute_keypoint_targets(np.zeros((0, 6), dtype=np.float32), cfg, gts, kps, info)
    assert rois.numpy().tolist() == [[0, 10, 20, 49, 59], [0, 100, 5, 163, 40]]
    row_of = lambda y, h: min(int(math.floor(y * 56 / h)), 55)      # noqa: E731
    assert targets[0].tolist() == [0, row_of(10, 40) * 56 + 55, -1, -1, 55 * 56 + row_of(20, 40), -1, -1]
    assert targets[1].tolist() == [rule((100, 5, 163, 40), k, 56, 56) for k in b] and (targets[1] >= 0).all()
    # windows of 1 x 1 and 1 x 300 pixels (the IoU without +1 never selects them; the rule itself must still hold)
    boxes = np.array([[7, 9, 7, 9], [7, 0, 7, 299]], dtype=np.int32)
    pts = np.array([[(7, 9, 2), (7.999, 9.999, 2), (8, 9, 2), (7, 8.5, 2)],
                    [(7.5, 0, 2), (7.5, below(300), 2), (7.5, 150, 2), (7.5, 300, 2)]], dtype=np.float64)
    got = keypoint_target_bins(boxes, pts, 56, 56)
    assert got.dtype == np.int32
    assert got.tolist() == [[rule(boxes[i], pts[i, k], 56, 56) for k in range(4)] for i in range(2)]
    assert got[0].tolist() == [0, 55 * 56 + 55, -1, -1] and got[1].tolist() == [28, 55 * 56 + 28, 28 * 56 + 28, -1]
    with pytest.raises(ValueError, match="ground_truth_keypoints"):
        compute_keypoint_targets(np.zeros((0, 6), dtype=np.float32), cfg, gts, kps[:, :2], info)


@pytest.mark.parametrize("name", list(mcases.CASES))
def test_selection_is_the_mask_targets_selection(name, cpu_backend):
    """same seed, same shared cfg keys: the same RoIs as compute_mask_targets, and numpy's global generator ends in the same state"""
    from scda_amd.dropin.functions.mask import compute_keypoint_targets, compute_mask_targets
    props, gts, masks, info, cfg = mcases.make(name)
    np.random.seed(11)
    mask_rois, _ = compute_mask_targets(torch.from_numpy(props), cfg, torch.from_numpy(gts), torch.from_numpy(masks), torch.from_numpy(info))
    after_mask = np.random.get_state()
    np.random.seed(11)
    rois, _ = compute_keypoint_targets(torch.from_numpy(props), kp_cfg(cfg), torch.from_numpy(gts), keypoints_for(gts, 5, 1),
                                       torch.from_numpy(info))
    after_kp = np.random.get_state()
    assert np.array_equal(rois.numpy(), mask_rois.numpy()[:, :5])
    assert after_kp[0] == after_mask[0] and np.array_equal(after_kp[1], after_mask[1]) and after_kp[2:] == after_mask[2:]


def test_round_trip_with_the_decode():
    """a heat map that is 1 at the target and 0 elsewhere decodes (host path: Pillow resize + argmax) to a pixel whose centre lies within
    max(roi_w / M_w, 1) x max(roi_h / M_h, 1) of the keypoint; a window at least as large as the map gives back the very bin"""
    from scda_amd.dropin.functions.mask import keypoint_target_bins, predict_keypoints
    M = 56
    rng = np.random.RandomState(21)
    sides = [1, 2, 3, 27, 55, 56, 57, 111, 112, 113, 300, 500] + rng.randint(1, 501, size=28).tolist()
    widths, heights = np.array(sides), np.array(sides[::-1])
    n, Kp = len(sides), 3
    x1, y1 = rng.randint(0, 40, n), rng.randint(0, 40, n)
    boxes = np.stack([x1, y1, x1 + widths - 1, y1 + heights - 1], 1).astype(np.int32)
    u = rng.uniform(0, 1, size=(n, Kp, 2))
    u[:, 0] = 0.0                                                                  # on (x1, y1)
    kps = np.concatenate([x1[:, None, None] + u[..., :1] * widths[:, None, None], y1[:, None, None] + u[..., 1:] * heights[:, None, None],
                          np.full((n, Kp, 1), 2.0)], axis=2)
    kps[:, 1, 0] = np.nextafter((x1 + widths).astype(np.float64), 0.0)             # just below (x2 + 1, y2 + 1)
    kps[:, 1, 1] = np.nextafter((y1 + heights).astype(np.float64), 0.0)
    targets = keypoint_target_bins(boxes, kps, M, M)
    assert (targets >= 0).all()
    heat = np.zeros((n, Kp, M * M), dtype=np.float32)
    np.put_along_axis(heat, targets[..., None].astype(np.int64), 1.0, axis=2)
    rois = np.concatenate([np.zeros((n, 1)), boxes], 1).astype(np.float32)
    got = predict_keypoints(rois, heat.reshape(n, Kp, M, M), np.array([[600, 600, 1.0]], dtype=np.float32))
    worst = 0.0
    for i in range(n):
        w, h = float(widths[i]), float(heights[i])
        for k in range(Kp):
            cx, cy = got[i, k, 0] + 0.5, got[i, k, 1] + 0.5
            ex, ey = abs(cx - kps[i, k, 0]) / max(w / M, 1.0), abs(cy - kps[i, k, 1]) / max(h / M, 1.0)
            worst = max(worst, ex, ey)
            assert ex <= 1.0 and ey <= 1.0, (boxes[i], kps[i, k], got[i, k])
            back = keypoint_target_bins(boxes[i:i + 1], np.array([[[cx, cy, 2.0]]]), M, M)[0, 0]
            if w >= M:
                assert back % M == targets[i, k] % M, (boxes[i], kps[i, k], got[i, k])
            if h >= M:
                assert back // M == targets[i, k] // M, (boxes[i], kps[i, k], got[i, k])
    print("round trip: worst distance %.3f of the bound" % worst)


def test_synth_keypoints_cover_the_interval_ends():
    from scda_amd import resnet_config as RC
    from scda_amd.dropin.functions.mask import keypoint_target_bins
    gts = torch.tensor([[[10., 20., 109., 99., 1.], [300., 40., 420., 200., 2.], [0., 0., 0., 0., 0.]]])
    kps = RC.synth_keypoints(gts, 17, seed=4)
    assert tuple(kps.shape) == (1, 3, 17, 3) and kps.dtype == torch.float32
    assert torch.equal(kps, RC.synth_keypoints(gts, 17, seed=4)) and not kps[0, 2].any()
    k = kps[0, :2].numpy().astype(np.float64)
    g = gts[0, :2].numpy()
    assert (k[:, :, 0] >= g[:, None, 0]).all() and (k[:, :, 0] < g[:, None, 2] + 1).all()
    assert (k[:, :, 1] >= g[:, None, 1]).all() and (k[:, :, 1] <= g[:, None, 3]).all()
    assert (k[:, 0, 0] == g[:, 0]).all() and (k[:, 1, 0] > g[:, 2] + 0.99).all()
    assert (k[..., 2] == 0).any() and (k[:, :2, 2] > 0).all()
    bins = keypoint_target_bins(g[:, :4].astype(np.int32), k, 56, 56)
    assert (bins[:, 0] % 56 == 0).all() and (bins[:, 1] % 56 == 55).all() and ((bins >= 0) == (k[..., 2] > 0)).all()
