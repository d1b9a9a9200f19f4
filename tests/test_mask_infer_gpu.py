"""Instance-mask inference on the MI355X (scda_amd/csrc/mask_ops.hip, scda_amd/infer.py masks=True): the resize-and-paste kernel
against the reference's golden predict_masks outputs and the host predict_masks bit for bit, the two small kernels against their numpy
statements, the whole path against the host composition, padding, batch invariance of the paste and graph replay."""
import os

import numpy as np
import pytest
import torch

import mask_cases as mcases
from gpu_arrays import dev as _dev, unpack as _unpack, words as _words
from test_mask_infer_rules import own_planes, pack_statement, paste_statement

pytestmark = pytest.mark.gpu


def sigmoid_statement(x):
    """scda_mask_select_hip's sigmoid: e = float32(exp(-x) in float64), then float32 add and divide"""
    e = np.exp(-x.astype(np.float64)).astype(np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)


def test_paste_equals_reference_golden(cuda, golden_dir):
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_masks_device
    rois, heat, info = mcases.predict_case()                                  # 14 x 14 planes on 60 x 80
    want = np.load(os.path.join(golden_dir, "mask_targets_ref.npz"))["predict_masks"]
    got = predict_masks_device(_dev(rois, cuda), _dev(heat, cuda), info)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    g = np.load(os.path.join(golden_dir, "predict_masks_sweep.npz"))          # 28 x 28 planes on 96 x 160
    rois, heat, info, want = g["rois"], g["heatmap"], g["image_info"], g["masks"]
    got = predict_masks_device(_dev(rois, cuda), _dev(heat, cuda), info).cpu().numpy()
    for r in range(rois.shape[0]):
        assert np.array_equal(got[r], want[r]), (r, rois[r])
    for thr in (0.0, 0.5):
        bits = N.mask_paste(_dev(rois, cuda), _dev(own_planes(heat, rois), cuda), 96, 160, packed=True, threshold=thr)
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (rois.shape[0], 96, 5)
        assert np.array_equal(_words(bits), pack_statement(want, thr))
    with pytest.raises(ValueError):
        predict_masks_device(_dev(rois, cuda), _dev(heat, cuda), np.array([[96, 160, 1.0], [96, 128, 1.0]]))


def _mixed_rois(rng, R, H, W):
    a, b, c = R // 4, R // 2, R - R // 4 - R // 2                            # small, medium, large (up to the full image)
    w = np.concatenate([rng.randint(1, 40, a), rng.randint(40, W // 3, b), rng.randint(W // 3, W + 1, c)])
    h = np.concatenate([rng.randint(1, 40, a), rng.randint(40, H // 3 + 1, b), rng.randint(H // 3, H + 1, c)])
    rng.shuffle(h)
    x1 = (rng.rand(R) * (W - w + 1)).astype(np.int64)
    y1 = (rng.rand(R) * (H - h + 1)).astype(np.int64)
    rois = np.stack([np.zeros(R), x1, y1, x1 + w - 1, y1 + h - 1, rng.rand(R), rng.randint(0, 9, R)], 1).astype(np.float32)
    rois[:, 1:5] += rng.rand(R, 4).astype(np.float32) * 0.9               # fractions that truncate
    rois[0, 1:5] = [0, 0, W - 1, H - 1]                                    # the whole image
    rois[1, 1:5] = [W - 28, H - 28, W - 1, H - 1]                          # 28 x 28 in the corner: both passes skipped
    return rois


def test_paste_equals_host_predict_masks_at_800x1344(cuda):
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_masks
    H, W, R = 800, 1344, 100
    rng = np.random.RandomState(31)
    rois = _mixed_rois(rng, R, H, W)
    heat = rng.rand(R, 9, 28, 28).astype(np.float32)
    info = np.array([[H, W, 1.0]], dtype=np.float32)
    planes = own_planes(heat, rois)
    got = N.mask_paste(_dev(rois, cuda), _dev(planes, cuda), H, W).cpu().numpy()
    for r0 in range(0, R, 20):
        want = predict_masks(rois[r0:r0 + 20], heat[r0:r0 + 20], info)
        for i, m in enumerate(want):
            assert np.array_equal(got[r0 + i], m), (r0 + i, rois[r0 + i])
    bits = _words(N.mask_paste(_dev(rois, cuda), _dev(planes, cuda), H, W, packed=True, threshold=0.5))
    assert bits.shape == (R, H, W // 32)
    assert np.array_equal(_unpack(bits, W), got >= 0.5)


def test_paste_odd_width_and_windows_that_leave_the_plane(cuda):
    """a width that is neither a multiple of 4 nor of 32, windows partly and wholly outside, empty windows, a padding row"""
    from scda_amd import native as N
    rng = np.random.RandomState(3)
    H, W = 70, 203
    rois = np.array([[0, -10, -5, 30, 20], [0, 150, 30, 260, 90], [0, 10, 10, 5, 20], [0, 300, 50, 400, 60], [0, 3, 3, 9, 9],
                     [0, 0, 0, 202, 69], [0, 120, 60, 140, 80], [0, np.inf, 0, 5, 5], [0, 100, 7, 131.9, 34.2]], dtype=np.float32)
    cls = np.array([1, 1, 1, 1, -1, 0, 2, 1, 1], dtype=np.int32)
    planes = rng.rand(rois.shape[0], 28, 28).astype(np.float32)
    want = paste_statement(rois, planes, H, W, cls=cls)
    got = N.mask_paste(_dev(rois, cuda), _dev(planes, cuda), H, W, cls=_dev(cls, cuda)).cpu().numpy()
    assert np.array_equal(got, want)
    assert not got[2].any() and not got[3].any() and not got[4].any() and not got[7].any() and got[0].any() and got[1].any()
    bits = N.mask_paste(_dev(rois, cuda), _dev(planes, cuda), H, W, cls=_dev(cls, cuda), packed=True, threshold=0.4)
    assert np.array_equal(_words(bits), pack_statement(want, 0.4))


def test_det_rois_and_mask_select_equal_their_statements(cuda):
    from scda_amd import native as N
    rng = np.random.RandomState(11)
    B, top_n, C = 3, 8, 9
    det = rng.rand(B, top_n, 7).astype(np.float32) * 30
    det[:, :, 3:5] += det[:, :, 1:3] + 2                                   # x2 > x1, y2 > y1, inside 64 x 100
    det[:, :, 6] = rng.randint(1, C, (B, top_n))
    counts = np.array([8, 0, 3], dtype=np.int32)
    rois, cls = N.det_rois(_dev(det, cuda), _dev(counts, cuda))
    want_r = np.zeros((B * top_n, 5), dtype=np.float32); want_c = -np.ones(B * top_n, dtype=np.int32)
    for b in range(B):
        want_r[b * top_n:(b + 1) * top_n, 0] = b
        want_r[b * top_n:b * top_n + counts[b], 1:5] = det[b, :counts[b], 1:5]
        want_c[b * top_n:b * top_n + counts[b]] = det[b, :counts[b], 6].astype(np.int32)
    assert np.array_equal(rois.cpu().numpy(), want_r) and np.array_equal(cls.cpu().numpy(), want_c)
    # class-plane select in both memory orders mask_predictor returns: NCHW, and the tall channel-major view transposed
    R = B * top_n
    logits = (rng.randn(R, C, 28, 28) * 3).astype(np.float32)
    nchw = _dev(logits, cuda)
    tall = _dev(logits.transpose(1, 0, 2, 3), cuda).view(C, R, 28, 28).transpose(0, 1)      # [R, C, 28, 28] view of [C, R*28, 28]
    assert not tall.is_contiguous() and torch.equal(tall, nchw)
    pick = np.where(want_c[:, None, None] >= 0, logits[np.arange(R), np.maximum(want_c, 0)], np.float32(0))
    for src in (nchw, tall):
        assert np.array_equal(N.mask_select(src, cls).cpu().numpy(), pick)
        got = N.mask_select(src, cls, sigmoid=True).cpu().numpy()
        assert np.array_equal(got, np.where(want_c[:, None, None] >= 0, sigmoid_statement(pick), np.float32(0)))
    assert not N.mask_select(nchw, cls, sigmoid=True)[top_n:2 * top_n].any()                 # the image without detections
    # padding rows and images without detections: all-zero words behind the paste
    bits = N.mask_paste(rois, N.mask_select(nchw, cls, sigmoid=True), 64, 100, cls=cls, packed=True)
    w = _words(bits).reshape(B, top_n, 64, 4)
    assert not w[1].any() and not w[2, 3:].any() and w[0].any() and w[2, :3].any()


def test_paste_batch_equals_single_images(cuda):
    """batch invariance of the paste kernel: a 2-image call against two 1-image calls on the same planes, bit for bit"""
    from scda_amd import native as N
    rng = np.random.RandomState(41)
    H, W, n = 128, 224, 30
    rois = np.concatenate([_mixed_rois(rng, n, H, W)[:, :5], _mixed_rois(rng, n, H, W)[:, :5]])
    rois[n:, 0] = 1
    planes = rng.rand(2 * n, 28, 28).astype(np.float32)
    cls = rng.randint(-1, 9, 2 * n).astype(np.int32)
    r_d, p_d, c_d = _dev(rois, cuda), _dev(planes, cuda), _dev(cls, cuda)
    for packed in (False, True):
        both = N.mask_paste(r_d, p_d, H, W, cls=c_d, packed=packed)
        for b in range(2):
            s = slice(b * n, (b + 1) * n)
            one = N.mask_paste(r_d[s].contiguous(), p_d[s].contiguous(), H, W, cls=c_d[s].contiguous(), packed=packed)
            assert torch.equal(both[s], one), (packed, b)
    assert np.array_equal(N.mask_paste(r_d, p_d, H, W, cls=c_d).cpu().numpy(), paste_statement(rois, planes, H, W, cls=cls))


# ---------------------------------------------------------------------------------------------------------------------------------
H_IMG, W_IMG = 256, 400            # W: a multiple of the stride, not of 32 (13 words per row, the last half used)
DET_SEED = 3


def _mask_detector(cuda, with_mask=True):
    """the detector's own initialisation under a fixed seed (an untrained detector: near-uniform class scores, top_n detections per
    image at score_thresh 0)"""
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    from test_resnet_oracle_gpu import CFG as RCFG
    torch.manual_seed(DET_SEED)
    det = resnet50(cfg=dict(RCFG['shared'], with_mask=with_mask))
    det = det.to(cuda).eval()
    if with_mask:
        _unit_logits(det, cuda)
    return det, RCFG


def _unit_logits(det, cuda):
    """Scale the mask head's output layer so that the logits of a fixed probe have unit standard deviation, as a trained head's do.
    The untrained stack (He-initialised convolutions, batch norms at their identity running statistics) gives logits in the hundreds:
    the sigmoid planes are then 0 / 1 steps, whose bicubic interpolation puts a share of every box at mid values, and a relative
    1e-6 between two convolution plans is an absolute 5e-4 (measured on the unscaled head: max |logit difference| 4.6e-4, 0.82 % of
    the box pixels within 4 x that of the threshold)."""
    with torch.no_grad():
        feat = det.feature_extractor(_images(70, 1, cuda))
        g = torch.Generator().manual_seed(70)
        x1 = torch.rand(16, generator=g) * (W_IMG - 120); y1 = torch.rand(16, generator=g) * (H_IMG - 120)
        rois = torch.stack([torch.zeros(16), x1, y1, x1 + 20 + torch.rand(16, generator=g) * 100, y1 + 20 + torch.rand(16, generator=g) * 100], 1)
        std = float(det.mask_predictor(feat, rois.to(cuda)).std())
        last = det.mask_head[-1]
        last.weight.mul_(1.0 / std)
        if last.bias is not None:
            last.bias.mul_(1.0 / std)


def _images(seed, B, cuda):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, H_IMG, W_IMG, generator=g) * 2 - 1).to(cuda)


def test_predictor_masks_equal_host_composition(cuda):
    """Predictor(masks=True), B = 2: the boxes are Predictor(masks=False)'s; every real detection's mask is the host composition
    (mask_predictor run eagerly per image on infer.rows' detections, the sigmoid, the host predict_masks, >= 0.5) except where the
    probability is within a margin of the threshold.  The margin is 4 x the measured max |logit difference| between the Predictor's
    head pass (R = 200 RoIs) and the eager per-image passes (R = 100 each: other convolution plans); the pixels inside it must be
    under 0.1 % of the pixels inside the boxes."""
    from scda_amd import infer
    from scda_amd.dropin.functions.mask import predict_masks
    det, cfg = _mask_detector(cuda)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.0]] * 2)
    pm = infer.Predictor(det, cfg, masks=True)
    out = [t.clone() for t in pm(x, info)]
    plain = infer.Predictor(det, cfg)(x, info)
    assert len(out) == 5 and len(plain) == 4
    for a, b in zip(out, plain):
        assert torch.equal(a, b)
    top_n = out[2].shape[1]
    assert out[4].dtype == torch.int32 and tuple(out[4].shape) == (2, top_n, H_IMG, (W_IMG + 31) // 32)
    _, dets = infer.rows(*out[:4])
    counts = out[3].cpu().numpy()
    assert counts.sum() == dets.shape[0] and counts.min() > 0
    got = infer.mask_rows(out[4], out[3], W_IMG)
    with torch.no_grad():
        feat = det.feature_extractor(x)
        inside = det.mask_predictor(feat, pm.mask_rois).detach().cpu().numpy()           # the Predictor's own pass, R = 2 * top_n
        start, max_diff, in_margin, in_boxes, wrong = 0, 0.0, 0, 0, 0
        eager = []
        for b in range(2):
            rows_b = dets[start:start + counts[b]]
            start += counts[b]
            logits = det.mask_predictor(feat, torch.from_numpy(rows_b[:, :5].copy()).to(cuda)).detach().cpu().numpy()
            max_diff = max(max_diff, float(np.abs(logits - inside[b * top_n:b * top_n + counts[b]]).max()))
            eager.append((rows_b, logits))
    margin = 4.0 * max_diff
    for b, (rows_b, logits) in enumerate(eager):
        prob = predict_masks(rows_b, sigmoid_statement(logits), info.numpy())
        assert got[b].shape == (counts[b], H_IMG, W_IMG)
        for r, p in enumerate(prob):
            x1, y1, x2, y2 = (int(v) for v in rows_b[r, 1:5])
            box = np.zeros_like(p, dtype=bool)
            box[y1:y2 + 1, x1:x2 + 1] = True
            near = np.abs(p - np.float32(0.5)) <= margin
            in_boxes += int(box.sum())
            in_margin += int((near & box).sum())
            wrong += int(((got[b][r] != (p >= 0.5)) & ~near).sum())
            assert not got[b][r][~box].any()
    print("max |logit difference| %.3e  margin %.3e  pixels in margin %d of %d in boxes (%.5f %%)  differing outside the margin %d"
          % (max_diff, margin, in_margin, in_boxes, 100.0 * in_margin / in_boxes, wrong))
    assert wrong == 0
    assert in_margin < 0.001 * in_boxes
    # infer.predict passes the argument through
    again = infer.predict(det, x, info, cfg, masks=True)
    assert len(again) == 5 and torch.equal(again[4], out[4])


def test_predictor_masks_replay_as_graph(cuda):
    from scda_amd import infer
    det, cfg = _mask_detector(cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.0]] * 2, device=cuda)
    sets = [_images(s, 2, cuda) for s in (81, 82, 83)]
    pred = infer.Predictor(det, cfg, masks=True)
    want = [[t.clone() for t in pred(y, info)] for y in sets]
    assert any(not torch.equal(want[0][4], w[4]) for w in want[1:])
    pred.capture(_images(84, 2, cuda), info)
    for y, w in zip(sets, want):
        pred.images.copy_(y)
        got = pred.replay()
        torch.cuda.synchronize()
        assert len(got) == 5
        for a, b in zip(got, w):
            assert torch.equal(a, b)


def test_predictor_masks_needs_the_mask_branch(cuda):
    from scda_amd import infer
    det, cfg = _mask_detector(cuda, with_mask=False)
    with pytest.raises(ValueError):
        infer.Predictor(det, cfg, masks=True)
    infer.Predictor(det, cfg)
