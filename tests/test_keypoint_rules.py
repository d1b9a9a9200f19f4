"""The keypoint branch at test time, host side (no GPU): the decode rule of include/scda_ops.h (scda_keypoint_decode_hip) as
dropin.functions.mask.predict_keypoints states it with PIL + numpy, against tests/golden/keypoints_ref.npz -- the REFERENCE's
predict_masks followed by np.argmax, which is what the rule is pinned to (the reference has no keypoint decoder of its own) --; its NaN
and padding rules against np.argmax directly; the model's branch (state_dict keys and shapes of the reference's), the refusal to train
it, the result writer and the Predictor's argument check."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_keypoints as gk  # noqa: E402

from test_host_functions import CFG  # noqa: E402

KP_CFG = dict(CFG['shared'], gan_model_flag=2, roi_align=True, with_keypoint=True, num_keypoints=17)


def golden(golden_dir):
    import PIL
    g = np.load(os.path.join(golden_dir, "keypoints_ref.npz"))
    if int(PIL.__version__.split(".")[0]) < 7:
        pytest.fail("the rule restates Pillow >= 7's BICUBIC float resize; this is Pillow %s" % PIL.__version__)
    return g


def test_host_rule_equals_reference_golden(golden_dir):
    from scda_amd.dropin.functions.mask import predict_keypoints
    g = golden(golden_dir)
    for name, case in (("sweep", gk.sweep_case), ("extra", gk.extra_case)):
        rois, heat, info = case()
        assert np.array_equal(rois[:, :5], g[name + "_boxes"])
        got = predict_keypoints(rois, heat, info)
        want = g[name]
        assert got.dtype == np.float32 and got.shape == want.shape
        for r in range(rois.shape[0]):
            assert np.array_equal(got[r].view(np.uint32), want[r].view(np.uint32)), (name, r, rois[r, 1:5], got[r], want[r])
    # what the extra planes are there for
    ex = g["extra"]
    for r, (x1, y1, x2, y2) in enumerate(gk.EXTRA_BOXES):
        assert tuple(ex[r, 0, :2]) == (x1, y1)                                 # the constant plane: row-major first
    assert tuple(ex[0, 1]) == (20 + 40, 10 + 10, 3.0)                          # identity: the first of three equal peaks
    assert (ex[:, 2, 2] < 0).all()                                             # all-negative: no zero from outside the window


def test_nan_padding_and_clipping_rules_against_argmax():
    from PIL import Image
    from scda_amd.dropin.functions.mask import predict_keypoints
    rng = np.random.RandomState(5)
    H, W = 60, 90
    heat = rng.randn(7, 2, 56, 56).astype(np.float32)
    heat[0, 0, 20, 30] = np.nan                                                # a NaN is a maximum (np.argmax), the first one wins
    heat[0, 0, 40, 10] = np.nan
    heat[0, 1, 3, 3] = np.inf
    rois = np.array([[0, 10, 2, 65, 57],                                       # 56 x 56: identity -> the NaN's own position
                     [0, -20, -10, 40, 30],                                    # partly outside, top-left
                     [0, 60, 40, 120, 80],                                     # partly outside, bottom-right
                     [0, 100, 10, 140, 30],                                    # wholly outside
                     [0, 30, 30, 20, 40],                                      # empty window
                     [0, np.nan, 0, 10, 10],                                   # not finite
                     [0, 5, 5, 25, 25]], dtype=np.float32)                     # a padding slot
    cls = np.array([1, 1, 1, 1, 1, 1, -1], dtype=np.int32)
    info = np.array([[H, W, 1.0]], dtype=np.float32)
    got = predict_keypoints(rois, heat, info, cls=cls)
    assert got[0, 0, 0] == 10 + 30 and got[0, 0, 1] == 2 + 20 and np.isnan(got[0, 0, 2])
    assert tuple(got[0, 1]) == (10 + 3, 2 + 3, np.inf)
    for r in (1, 2):
        x1, y1, x2, y2 = (int(v) for v in rois[r, 1:5])
        for k in range(2):
            m = np.array(Image.fromarray(heat[r, k]).resize((x2 - x1 + 1, y2 - y1 + 1)))
            full = np.full((H + 200, W + 200), -np.inf, dtype=np.float32)      # the window on a larger canvas, then the image cut out
            full[100 + y1:100 + y2 + 1, 100 + x1:100 + x2 + 1] = m
            seen = full[100:100 + H, 100:100 + W]
            at = np.argmax(seen)
            assert tuple(got[r, k]) == (at % W, at // W, seen.reshape(-1)[at])
    assert not got[3:].any()
    assert predict_keypoints(rois, heat, info)[6].any()                        # without cls the last row is a real one


def test_model_branch_has_the_reference_state_dict():
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    plain = resnet50(cfg=dict(KP_CFG, with_keypoint=False))
    det = resnet50(cfg=KP_CFG)
    assert det.with_keypoint and det.num_keypoints == 17 and not plain.with_keypoint
    want = {}
    for i in range(8):
        want["keypoint_head.%d.0.weight" % i] = (512, 1024 if i == 0 else 512, 3, 3)
        want["keypoint_head.%d.0.bias" % i] = (512,)
    want["keypoint_head.8.0.weight"] = (512, 512, 2, 2)
    want["keypoint_head.8.0.bias"] = (512,)
    want["keypoint_head.10.weight"] = (17, 512, 1, 1)
    want["keypoint_head.10.bias"] = (17,)
    sd = det.state_dict()
    got = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("keypoint")}
    assert got == want
    assert set(sd) - set(got) == set(plain.state_dict())                       # nothing else appears or moves
    assert len(det.keypoint_head) == 11 and not list(det.keypoint_head[9].parameters())


def test_trainer_refuses_a_detector_with_the_keypoint_branch():
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    from scda_amd.train_step import ScdaTrainer
    det = resnet50(cfg=KP_CFG)
    with pytest.raises(ValueError, match="keypoint"):
        ScdaTrainer(CFG, torch.device("cpu"), models=(det, None, None, None))


def test_predictor_needs_the_keypoint_branch():
    from scda_amd import infer
    from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
    det = resnet50(cfg=dict(KP_CFG, with_keypoint=False)).eval()
    with pytest.raises(ValueError, match="keypoint"):
        infer.Predictor(det, CFG, keypoints=True)
    infer.Predictor(det, CFG)


class _Evaluator:
    iou_type, D, Kp, use_cats = 'keypoints', 100, 17, True


class _Predictor:
    keypoints, masks, rle, original_size = False, False, False, None


def test_coco_stats_names_the_missing_argument():
    from scda_amd import evaluate
    with pytest.raises(ValueError, match="keypoints=True"):
        evaluate.coco_stats([], _Predictor(), _Evaluator())


def test_write_keypoint_results_lines():
    from scda_amd import evaluate
    rng = np.random.RandomState(9)
    B, top_n, Kp = 2, 5, 3
    det = np.zeros((B, top_n, 7), dtype=np.float32)
    det[:, :, 1:3] = rng.rand(B, top_n, 2) * 50
    det[:, :, 3:5] = det[:, :, 1:3] + 10 + rng.rand(B, top_n, 2) * 40
    det[:, :, 5] = rng.rand(B, top_n)
    det[0, 1, 5] = det[0, 3, 5]                                                # a tie: the detections' order decides
    det[:, :, 6] = rng.randint(1, 9, (B, top_n))
    counts = np.array([5, 2], dtype=np.int32)
    scale = np.array([1.5, 0.8], dtype=np.float32)
    kp = (rng.rand(B, top_n, Kp, 3) * 90).astype(np.float32)
    kpo = kp.copy()
    kpo[..., :2] /= scale[:, None, None, None]
    info = np.stack([np.full(B, 100.0), np.full(B, 160.0), scale], 1).astype(np.float32)
    out = tuple(torch.from_numpy(a) for a in (np.zeros((B, 3, 6), np.float32), np.zeros(B, np.int32), det, counts, kp, kpo))
    buf = io.StringIO()
    evaluate.write_keypoint_results(buf, info, [7, 9], out, category_of=lambda c: c + 100, keep_num=4)
    lines = [json.loads(s) for s in buf.getvalue().splitlines()]
    assert len(lines) == 4 + 2
    want_order = [(0, i) for i in np.argsort(-det[0, :5, 5], kind='stable')[:4]] + [(1, i) for i in np.argsort(-det[1, :2, 5], kind='stable')]
    for line, (b, i) in zip(lines, want_order):
        box = (det[b, i, 1:5] / scale[b]).tolist()
        assert line == {'image_id': [7, 9][b], 'bbox': [box[0], box[1], box[2] - box[0], box[3] - box[1]], 'score': det[b, i, 5].tolist(),
                        'category_id': int(det[b, i, 6]) + 100, 'keypoints': kpo[b, i].reshape(-1).tolist()}
        assert len(line['keypoints']) == 3 * Kp
    with pytest.raises(ValueError):
        evaluate.write_keypoint_results(io.StringIO(), info[:, :2], [7, 9], out)
    with pytest.raises(ValueError):
        evaluate.write_keypoint_results(io.StringIO(), info, [7, 9], out[:4])
