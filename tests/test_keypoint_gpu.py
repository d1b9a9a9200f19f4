"""The keypoint branch at test time on the MI355X: the decode kernel (scda_amd/csrc/keypoint_ops.hip) against
tests/golden/keypoints_ref.npz -- the reference's predict_masks + np.argmax, what the rule is pinned to -- and against the host rule
(dropin.functions.mask.predict_keypoints) bit for bit; model.keypoint_predictor (tall against NCHW, the up-sampling seam, accuracy
against a float64 composition on the CPU); Predictor(keypoints=True) against the host rule on its own heat maps, and graph replay;
evaluate.coco_stats with a 'keypoints' evaluator against CocoEvaluator.add fed by hand."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_keypoints as gk  # noqa: E402
from gpu_arrays import bits as _bits, dev as _dev  # noqa: E402

pytestmark = pytest.mark.gpu

KP = 17


def _tall(heat, cuda):
    """[R, Kp, h, w] on the host -> the same values as the transposed view of a channel-major [Kp, R*h, w] stack on the device"""
    R, Kp, h, w = heat.shape
    t = _dev(heat.transpose(1, 0, 2, 3), cuda).view(Kp, R, h, w).transpose(0, 1)
    assert not t.is_contiguous() and tuple(t.shape) == heat.shape
    return t


def test_decode_equals_reference_golden(cuda, golden_dir):
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_keypoints_device
    g = np.load(os.path.join(golden_dir, "keypoints_ref.npz"))
    for name, case in (("sweep", gk.sweep_case), ("extra", gk.extra_case)):
        rois, heat, info = case()
        want = g[name]
        Hh, Ww = int(info[0, 0]), int(info[0, 1])
        for src in (_dev(heat, cuda), _tall(heat, cuda)):
            got = N.keypoint_decode(_dev(rois, cuda), src, Hh, Ww).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == want.shape
            for r in range(rois.shape[0]):
                assert np.array_equal(_bits(got[r]), _bits(want[r])), (name, src.is_contiguous(), r, rois[r, 1:5], got[r], want[r])
        got = predict_keypoints_device(_dev(rois, cuda), _dev(heat, cuda), info).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):
        predict_keypoints_device(_dev(rois, cuda), _dev(heat, cuda), np.array([[128, 200, 1.0], [128, 160, 1.0]]))


def test_decode_rows_equal_the_host_rule(cuda):
    """what needs no fixture: windows partly and wholly outside (H, W), a padding slot, cls = None, a coordinate that is not finite, a
    NaN in a heat map, 64 x 64 planes (65 refused), R = 1 with Kp = 1"""
    from scda_amd import native as N
    from scda_amd.dropin.functions.mask import predict_keypoints
    rng = np.random.RandomState(13)
    Hh, Ww = 70, 203                                                           # two strips, the second partly used
    rois = np.array([[0, -10, -5, 30, 20], [0, 150, 30, 260, 90], [0, 10, 10, 5, 20], [0, 300, 50, 400, 60], [0, 3, 3, 9, 9],
                     [0, 0, 0, 202, 69], [0, 120, 60, 140, 80], [0, np.inf, 0, 5, 5], [0, 100, 7, 131.9, 34.2],
                     [0, 60, 2, 115, 57], [0, 100, 1, 180, 40]], dtype=np.float32)
    cls = np.array([1, 1, 1, 1, -1, 0, 2, 1, 1, 1, 3], dtype=np.int32)
    info = np.array([[Hh, Ww, 1.0]], dtype=np.float32)
    heat = rng.randn(rois.shape[0], 2, 56, 56).astype(np.float32)
    heat[9, 0, 17, 21] = np.nan                                                # in the identity window and in a resized one
    heat[10, 1, 30, 30] = np.nan
    heat[10, 1, 31, 5] = np.nan
    for c in (cls, None):
        want = predict_keypoints(rois, heat, info, cls=c)
        got = N.keypoint_decode(_dev(rois, cuda), _dev(heat, cuda), Hh, Ww, cls=None if c is None else _dev(c, cuda)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
        assert not got[2].any() and not got[3].any() and not got[7].any() and got[0].any() and got[1].any()
        assert got[4].any() == (c is None)
    assert np.isnan(want[9, 0, 2]) and tuple(want[9, 0, :2]) == (60 + 21, 2 + 17) and np.isnan(want[10, 1, 2])
    # the largest planes: 64 x 64, up- and down-scaled on either axis, the identity, one pass skipped
    rois = np.array([[0, 5, 5, 68, 68], [0, 0, 0, 202, 69], [0, 30, 10, 60, 50], [0, 100, 3, 163, 30], [0, 10, 1, 30, 64],
                     [0, 150, 20, 202, 69], [0, 7, 9, 7, 9]], dtype=np.float32)
    heat = rng.randn(rois.shape[0], 2, 64, 64).astype(np.float32)
    want = predict_keypoints(rois, heat, info)
    for src in (_dev(heat, cuda), _tall(heat, cuda)):
        got = N.keypoint_decode(_dev(rois, cuda), src, Hh, Ww).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
    big = torch.zeros(2, 1, 65, 64, device=cuda)
    with pytest.raises(ValueError):
        N.keypoint_decode(_dev(rois[:2], cuda), big, Hh, Ww)
    ws = torch.empty(4096, dtype=torch.uint8, device=cuda)                    # the entry point itself refuses too: a status, no launch
    out = torch.zeros(2, 1, 3, device=cuda)
    r2 = _dev(rois[:2], cuda)
    for ph, pw in ((65, 64), (64, 65)):
        assert N.lib().scda_keypoint_decode_hip(r2.data_ptr(), 5, None, big.data_ptr(), 65 * 64, 65 * 64, 64, 1, 2, 1, ph, pw, Hh, Ww,
                                                ws.data_ptr(), out.data_ptr(), None) != 0
    # R = 1, Kp = 1
    one = rng.randn(1, 1, 56, 56).astype(np.float32)
    roi = np.array([[0, 20, 11, 150, 66]], dtype=np.float32)
    got = N.keypoint_decode(_dev(roi, cuda), _dev(one, cuda), Hh, Ww).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(predict_keypoints(roi, one, info)))


# --------------------------------------------------------------------------------------------------------------- the head
def _detector(cuda, seed=3):
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    from test_resnet_oracle_gpu import CFG as RCFG
    torch.manual_seed(seed)
    det = resnet50(cfg=dict(RCFG['shared'], with_keypoint=True, num_keypoints=KP)).to(cuda).eval()
    return det, RCFG


_HEAD = {}


def _head_case(cuda):
    """one detector, one [1, 1024, 16, 24] feature map and 8 RoIs, with the float64 and float32 CPU compositions of the branch (computed
    once, shared and left unchanged)"""
    if _HEAD:
        return _HEAD
    import roi_refs
    det, _ = _detector(cuda)
    g = torch.Generator().manual_seed(8)
    feat = torch.randn(1, 1024, 16, 24, generator=g) * 0.5
    x1 = torch.rand(8, generator=g) * 250; y1 = torch.rand(8, generator=g) * 150
    rois = torch.stack([torch.zeros(8), x1, y1, x1 + 20 + torch.rand(8, generator=g) * 110, y1 + 20 + torch.rand(8, generator=g) * 80], 1)
    # RoIAlignAvg(14, 14): a 15 x 15 sample grid, then the 2 x 2 average at stride 1
    aligned = torch.from_numpy(roi_refs.roi_align(feat.numpy(), rois.numpy(), 15, 15, 1.0 / 16))
    sd = {k: v.detach().cpu() for k, v in det.keypoint_head.state_dict().items()}

    def compose(dtype):
        x = F.avg_pool2d(aligned.to(dtype), kernel_size=2, stride=1)
        for i in range(8):
            x = F.relu(F.conv2d(x, sd["%d.0.weight" % i].to(dtype), sd["%d.0.bias" % i].to(dtype), padding=1))
        x = F.relu(F.conv_transpose2d(x, sd["8.0.weight"].to(dtype), sd["8.0.bias"].to(dtype), stride=2))
        x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True)
        return F.conv2d(x, sd["10.weight"].to(dtype), sd["10.bias"].to(dtype))

    with torch.no_grad():
        _HEAD.update(det=det, feat=feat.to(cuda), rois=rois.to(cuda), ref64=compose(torch.float64), ref32=compose(torch.float32))
    return _HEAD


def _errors(y, ref64):
    d = y.detach().cpu().double() - ref64
    rms = ref64.pow(2).mean().sqrt().item()
    return d.abs().max().item() / rms, d.pow(2).mean().sqrt().item() / rms


def close(a, b, tol):
    """tests/test_resnet_gpu.py's measure for the channel-major RoI head: the largest difference relative to the largest value"""
    err = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
    assert err < tol, "relative-to-max error %.3e" % err
    return err


def test_keypoint_predictor_tall_equals_nchw_and_has_no_seam(cuda, monkeypatch):
    c = _head_case(cuda)
    det, feat, rois = c['det'], c['feat'], c['rois']
    with torch.no_grad():
        tall = det.keypoint_predictor(feat, rois)
        assert det.keypoint_roipooling.channel_major and tuple(tall.shape) == (8, KP, 56, 56) and not tall.is_contiguous()
        tall = tall.clone()
        six = det.keypoint_predictor(feat, rois[:6].contiguous())                          # R % 4 != 0: the NCHW path
        assert not det.keypoint_roipooling.channel_major and tuple(six.shape) == (6, KP, 56, 56) and six.is_contiguous()
        # the seam: RoI 3's input changes, RoI 2's maps (and every other's) keep their bits
        moved = rois.clone()
        moved[3, 1:5] = torch.tensor([5.0, 9.0, 300.0, 200.0], device=cuda)
        other = det.keypoint_predictor(feat, moved)
        assert not torch.equal(other[3], tall[3])
        for r in (0, 1, 2, 4, 5, 6, 7):
            assert torch.equal(other[r], tall[r]), r
        monkeypatch.setenv("SCDA_RESNET_HEAD_NCHW", "1")
        nchw = det.keypoint_predictor(feat, rois)
        assert not det.keypoint_roipooling.channel_major and nchw.is_contiguous()
    # 2e-4: what test_channel_major_roi_head_equals_reference_layout allows the default build (Winograd against the direct kernel)
    print("tall against NCHW: relative-to-max error %.3e; R = 6 against R = 8 (NCHW) %.3e"
          % (close(tall, nchw, 2e-4), close(six, nchw[:6], 2e-4)))


def test_keypoint_predictor_accuracy_against_float64(cuda):
    """the device error against the float64 composition (tests/roi_refs.py RoIAlign, F.conv2d, F.conv_transpose2d, F.interpolate with
    align_corners=True), max and rms relative to the output's rms, within FACTOR['wino'] = 4 (tests/test_conv_edges_gpu.py: what a
    Winograd launch is allowed over fp32 direct sums) of the same composition evaluated in float32 on the CPU"""
    from test_conv_edges_gpu import FACTOR
    c = _head_case(cuda)
    with torch.no_grad():
        got = {"tall": c['det'].keypoint_predictor(c['feat'], c['rois']).clone(),
               "nchw R = 6": c['det'].keypoint_predictor(c['feat'], c['rois'][:6].contiguous())}
    e32 = _errors(c['ref32'], c['ref64'])
    print("keypoint head, [1, 1024, 16, 24] features, 8 RoIs, Kp = 17: error against float64 relative to the output's rms")
    print("  float32 on the CPU     max %.3e  rms %.3e" % e32)
    for name, y in got.items():
        ref = c['ref64'][:y.shape[0]]
        e = _errors(y, ref)
        print("  device, %-12s   max %.3e  rms %.3e   (allowed: %.0f x the float32 figures)" % (name, e[0], e[1], FACTOR['wino']))
        assert e[0] <= FACTOR['wino'] * e32[0] and e[1] <= FACTOR['wino'] * e32[1], (name, e, e32)


# ---------------------------------------------------------------------------------------------------------- the Predictor
H_IMG, W_IMG = 256, 400                                                        # tests/test_mask_infer_gpu.py's
TOP_N = 20


def _images(seed, B, cuda):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, H_IMG, W_IMG, generator=g) * 2 - 1).to(cuda)


_PRED = {}


def _predictor(cuda):
    if not _PRED:
        from scda_amd import infer
        det, cfg = _detector(cuda)
        cfg = copy.deepcopy(cfg)
        cfg['test_predict_bbox_cfg']['top_n'] = TOP_N
        _PRED.update(det=det, cfg=cfg, pred=infer.Predictor(det, cfg, keypoints=True))
    return _PRED['det'], _PRED['cfg'], _PRED['pred']


def _host_rows(det_rows, counts):
    B, top_n = det_rows.shape[:2]
    rois = np.zeros((B * top_n, 5), dtype=np.float32)
    cls = -np.ones(B * top_n, dtype=np.int32)
    for b in range(B):
        rois[b * top_n:(b + 1) * top_n, 0] = b
        rois[b * top_n:b * top_n + counts[b], 1:5] = det_rows[b, :counts[b], 1:5]
        cls[b * top_n:b * top_n + counts[b]] = det_rows[b, :counts[b], 6].astype(np.int32)
    return rois, cls


def test_predictor_keypoints_equal_the_host_rule_on_its_own_heat_maps(cuda):
    from scda_amd import infer
    from scda_amd.dropin.functions.mask import predict_keypoints
    det, cfg, pred = _predictor(cuda)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.5], [H_IMG, W_IMG, 0.75]])
    out = [t.clone() for t in pred(x, info)]
    heat = pred.keypoint_heat.cpu().numpy()
    plain = infer.Predictor(det, cfg)(x, info)
    assert len(out) == 6 and len(plain) == 4
    for a, b in zip(out, plain):
        assert torch.equal(a, b)
    kp, kpo = out[4].cpu().numpy(), out[5].cpu().numpy()
    assert kp.dtype == np.float32 and kp.shape == (2, TOP_N, KP, 3) and kpo.shape == kp.shape and heat.shape == (2 * TOP_N, KP, 56, 56)
    counts = out[3].cpu().numpy()
    assert counts.min() > 0
    rois, cls = _host_rows(out[2].cpu().numpy(), counts)
    want = predict_keypoints(rois, heat, np.array([[H_IMG, W_IMG]] * 2), cls=cls).reshape(kp.shape)
    assert np.array_equal(_bits(kp), _bits(want))
    want_o = want.copy()
    want_o[..., 0:2] = want[..., 0:2] / info.numpy()[:, 2].reshape(2, 1, 1, 1)
    assert np.array_equal(_bits(kpo), _bits(want_o))
    for b in range(2):
        assert not kp[b, counts[b]:].any() and not kpo[b, counts[b]:].any()
        assert kp[b, :counts[b], :, 0].max() > 0                               # and the real rows are not trivially zero
    again = infer.predict(det, x, info, cfg, keypoints=True)
    assert len(again) == 6 and torch.equal(again[4], out[4]) and torch.equal(again[5], out[5])
    with pytest.raises(ValueError):
        pred(x, info[:, :2])
    # one capture / replay returns the same bytes
    pred(x, info)
    pred.capture(_images(84, 2, cuda), info.to(cuda))
    pred.images.copy_(x)
    got = pred.replay()
    torch.cuda.synchronize()
    assert len(got) == 6
    for a, b in zip(got, out):
        assert torch.equal(a, b)


def test_coco_stats_with_a_keypoint_evaluator_equals_feeding_add_by_hand(cuda):
    from scda_amd import evaluate
    from scda_amd.coco_eval import CocoEvaluator
    det, cfg, pred = _predictor(cuda)
    G, K = 4, 8
    info = torch.tensor([[H_IMG, W_IMG, 1.25], [H_IMG, W_IMG, 0.8]])
    rng = np.random.RandomState(17)
    items, fed = [], []
    for n, seed in enumerate((91, 92)):
        x = _images(seed, 2, cuda)
        out = [t.clone() for t in pred(x, info)]
        d, kp = out[2].cpu().numpy(), out[4].cpu().numpy()
        gb, ga = np.zeros((2, G, 4)), np.zeros((2, G))
        gi, gc, gn = np.zeros((2, G), np.uint8), np.zeros((2, G), np.int32), np.zeros((2, G), np.int32)
        gk = np.zeros((2, G, KP, 3))
        for b in range(2):                                                     # ground truth near some of the detections
            for g_ix, j in enumerate((0, 3, 7, 12)):
                x1, y1, x2, y2 = d[b, j, 1:5].astype(np.float64)
                gb[b, g_ix] = (x1, y1, x2 - x1, y2 - y1)
                ga[b, g_ix] = gb[b, g_ix, 2] * gb[b, g_ix, 3]
                gi[b, g_ix], gc[b, g_ix] = g_ix == 2, int(d[b, j, 6])
                gk[b, g_ix, :, :2] = kp[b, j, :, :2] + rng.randn(KP, 2) * 3
                gk[b, g_ix, :, 2] = rng.randint(0, 3, KP)
                gn[b, g_ix] = int((gk[b, g_ix, :, 2] > 0).sum())
        gt = dict(gt_boxes=_dev(gb, cuda), gt_areas=_dev(ga, cuda), gt_iscrowd=_dev(gi, cuda), gt_categories=_dev(gc, cuda),
                  gt_counts=_dev(np.full(2, G, np.int32), cuda), gt_keypoints=_dev(gk, cuda), gt_num_keypoints=_dev(gn, cuda))
        ids = torch.tensor([10 + 2 * n, 11 + 2 * n], dtype=torch.int32)
        items.append(dict(gt, image=x, image_info=info, image_ids=ids))
        fed.append((ids, out, gt))
    new = lambda: CocoEvaluator(K, 'keypoints', num_keypoints=KP, max_images=4, max_dets_per_image=TOP_N, max_gts_per_image=G,   # noqa: E731
                                device=cuda)
    for orig in (False, True):
        stats = evaluate.coco_stats(items, pred, new(), original_keypoints=orig)
        ev = new()
        for ids, out, gt in fed:
            ev.add(ids, out[2], out[3], gt['gt_boxes'], gt['gt_areas'], gt['gt_iscrowd'], gt['gt_categories'], gt['gt_counts'],
                   keypoints=out[5] if orig else out[4], gt_keypoints=gt['gt_keypoints'], gt_num_keypoints=gt['gt_num_keypoints'])
        want = ev.summarize()
        print("keypoint stats (original_keypoints=%s)" % orig, stats)
        assert stats.shape == (10,) and np.array_equal(stats.view(np.uint64), want.view(np.uint64))
    assert stats[0] != -1
    with pytest.raises(ValueError):                                            # D and Kp must be the Predictor's
        evaluate.coco_stats(items, pred, CocoEvaluator(K, 'keypoints', num_keypoints=KP, max_images=4, max_dets_per_image=TOP_N + 1,
                                                       max_gts_per_image=G, device=cuda))
