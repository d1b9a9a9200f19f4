"""Soft-NMS on the MI355X (scda_amd/csrc/soft_nms.hip): the kernel against the reference's compiled soft_nms on every fixture case
(tests/golden/soft_nms_ref.npz; tests/test_soft_nms.py holds the host loop to the same cases), method 0 against the hard NMS kernel,
box_predict and the Predictor with the soft sweep against the host composition / the eval forward's own box prediction, all bit for
bit, and the capacity's refusal."""
import os

import numpy as np
import pytest
import torch

import nms_cases
import soft_nms_cases as sc
import soft_nms_refs as refs
from test_host_functions import CFG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture_cases(golden_dir):
    return sc.load(os.path.join(golden_dir, "soft_nms_ref.npz"))


def _pack(lists, empty_at):
    """lists back to back with one EMPTY segment at list position `empty_at` -> boxes [rows,5], seg [S,3] (the third column unused)"""
    lens = [len(a) for a in lists]
    lens.insert(empty_at, 0)
    seg = np.zeros((len(lens), 3), dtype=np.int64)
    seg[:, 1] = lens
    seg[1:, 0] = np.cumsum(lens)[:-1]
    return np.concatenate(lists, 0), seg


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("pi", range(len(sc.PARAMS)))
def test_kernel_equals_reference_bit_for_bit(cuda, fixture_cases, method, pi):
    """all cases of one (method, parameter set) as the segments of ONE launch (lengths 1 .. 300, with 2048 where the fixture has it,
    and an empty segment among them): counts, kept indices in selection order and the kept rows' score bits are the reference's;
    a second run on a fresh copy writes the same bytes"""
    from scda_amd import native as N
    sigma, Nt, threshold = sc.PARAMS[pi]
    cases = fixture_cases[(method, pi)]
    empty_at = 5
    packed, seg = _pack([c[1] for c in cases], empty_at)
    max_n = int(seg[:, 1].max())
    runs = []
    for _ in range(2):
        b = torch.from_numpy(packed).to(cuda)
        keep, num = N.soft_nms_segments(b, torch.from_numpy(seg).to(cuda), max_n, method, sigma, Nt, threshold)
        runs.append((b.cpu().numpy(), keep.cpu().numpy(), num.cpu().numpy()))
    boxes, keep, num = runs[0]
    assert num[empty_at] == 0
    np.testing.assert_array_equal(boxes[:, :4].view(np.uint32), packed[:, :4].view(np.uint32))          # only the score column is written
    rows = [s for i, s in enumerate(seg) if i != empty_at]
    nums = np.delete(num, empty_at)
    for (name, _, want_boxes, want_inds), (first, n, _), k in zip(cases, rows, nums):
        assert k == len(want_inds), name
        got_inds = keep[first:first + k]
        np.testing.assert_array_equal(got_inds, want_inds, err_msg=name)
        np.testing.assert_array_equal(boxes[first + got_inds].view(np.uint32), want_boxes.view(np.uint32), err_msg=name)
    assert runs[1][0].tobytes() == boxes.tobytes() and np.array_equal(runs[1][2], num)
    for (first, n, _), k in zip(seg, num):
        assert np.array_equal(runs[1][1][first:first + k], keep[first:first + k])


def test_method_0_keeps_what_hard_nms_keeps(cuda):
    """rpn_300_t07 (no pair on its threshold, every score above 0.001): the soft sweep's hard rule at Nt = the case's threshold
    keeps the set native.nms keeps"""
    from scda_amd import native as N
    dets = nms_cases.make("rpn_300_t07")
    thresh = next(c for c in nms_cases.CASES if c[0] == "rpn_300_t07")[3]
    hk, hn = N.nms(torch.from_numpy(dets).to(cuda), thresh)
    b = torch.from_numpy(dets).to(cuda)
    seg = torch.tensor([[0, len(dets), 0]], dtype=torch.int64, device=cuda)
    sk, sn = N.soft_nms_segments(b, seg, len(dets), 0, 0.5, thresh, 0.001)
    hard, soft = hk[:int(hn)].cpu().numpy(), sk[:int(sn[0])].cpu().numpy()
    assert 0 < len(hard) < len(dets)
    np.testing.assert_array_equal(np.sort(soft), np.sort(hard))
    np.testing.assert_array_equal(soft, hard)                           # sorted input: selection order = score order = index order
    np.testing.assert_array_equal(b.cpu().numpy()[soft].view(np.uint32), dets[soft].view(np.uint32))    # weight 1: scores as they were


def _box_predict(cuda, head, cfg, soft, top_n):
    from scda_amd import native as N
    rois, counts, prob, loc, info = head
    B, P, C = len(counts), rois.shape[0] // len(counts), prob.shape[1]
    det = torch.full((B, top_n, 7), -7.0, device=cuda)
    dc = torch.full((B,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty(N.box_predict_workspace_bytes(B, P, C), dtype=torch.uint8, device=cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)      # noqa: E731
    N.box_predict(t(rois), t(counts), t(prob), t(loc), t(info), cfg['bbox_normalize_stds'], cfg['bbox_normalize_means'],
                  cfg['score_thresh'], cfg['nms_iou_thresh'], top_n, ws, det, dc, soft_nms=soft)
    return det.cpu().numpy(), dc.cpu().numpy()


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("top_n", [40, 10])
def test_box_predict_with_soft_nms_equals_the_host_composition(cuda, method, top_n):
    """B = 2, P = 64, C = 4: image 1 holds 37 real rows, class 2 is empty, a score threshold cuts the lists; rows and counts are the
    plain numpy composition's (decode, clip, threshold, sort, soft_nms, top-n), bit for bit"""
    soft = refs.SETTINGS[method]
    cfg = dict(CFG["test_predict_bbox_cfg"], score_thresh=0.05, top_n=top_n)
    head = refs.synth_head(seed=3)
    rois, counts, prob, loc, info = head
    real = refs.real_rows(counts, 64)
    want = refs.predict_rows(rois[real], prob[real], loc[real], info, cfg, soft)
    det, dc = _box_predict(cuda, head, cfg, soft, top_n)
    for b in range(2):
        w = want[want[:, 0] == b]
        assert dc[b] == len(w) > 0
        np.testing.assert_array_equal(det[b, :dc[b]].view(np.uint32), w.view(np.uint32))
        assert (det[b, dc[b]:] == 0).all()
    hard_det, _ = _box_predict(cuda, head, cfg, None, top_n)
    assert not np.array_equal(hard_det, det)                             # and the argument is what switches


def _detector(cuda):
    from test_infer_gpu import _detector as d
    return d(cuda)


def test_predictor_with_soft_nms(cuda, monkeypatch):
    """Predictor(model, cfg, soft_nms=...) at 200 x 312, two images: the detections are the rows the eval forward's own box prediction
    (compute_predicted_bboxes with the cfg key set) gives on the SAME proposals and head outputs -- recorded where the Predictor
    hands them to box_predict, because the eval forward's RPN decode evaluates exp with numpy's float32 routine and its proposals may
    differ from the device's in their last bits (include/scda_ops.h); the untrained detector's head gives some twenty RoIs per class a
    score another RoI has too, so the rows also pin that both paths order equal scores by one rule --, the cfg key alone gives the same bytes as the argument,
    capture + replay returns them again, and soft_nms=None is a Predictor built without the argument, byte for byte"""
    from test_eval_path import si
    from scda_amd import infer
    from scda_amd import native as N
    from scda_amd.dropin.functions.predict_bbox import compute_predicted_bboxes
    det = _detector(cuda)
    H, W = 200, 312
    imgs = torch.cat([si.synth_images(s, H, W)[0] for s in (51, 52)], 0).to(cuda)
    info = torch.tensor([[H, W, 1.0]] * 2)
    soft = refs.SETTINGS[1]
    cfg_soft = {k: dict(v) for k, v in CFG.items()}
    cfg_soft["test_predict_bbox_cfg"]["soft_nms"] = soft

    seen = {}
    real_box_predict = N.box_predict

    def recording(rois, counts, prob, loc, *a, **kw):
        seen.update(rois=rois.cpu().numpy(), counts=counts.cpu().numpy(), prob=prob.cpu().numpy(), loc=loc.cpu().numpy(), soft=kw['soft_nms'])
        return real_box_predict(rois, counts, prob, loc, *a, **kw)

    pred = infer.Predictor(det, CFG, soft_nms=soft)
    with monkeypatch.context() as m:
        m.setattr(N, "box_predict", recording)
        out = [t.clone() for t in pred(imgs, info)]
    assert seen['soft'] == (1, 0.5, 0.3, 0.001)
    _, got = infer.rows(*out)
    real = refs.real_rows(seen['counts'], pred.P)
    want = compute_predicted_bboxes(torch.from_numpy(seen['rois'][real]), torch.from_numpy(seen['prob'][real]),
                                    torch.from_numpy(seen['loc'][real]), info.numpy(), cfg_soft["test_predict_bbox_cfg"]).numpy()
    assert got.shape == want.shape and got.shape[0] > 0
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # the cfg key alone
    by_key = infer.Predictor(det, cfg_soft)(imgs, info)
    for a, b in zip(by_key, out):
        assert torch.equal(a, b)
    # capture + replay
    pred.capture(imgs, info)
    again = pred.replay()
    torch.cuda.synchronize()
    for a, b in zip(again, out):
        assert torch.equal(a, b)
    # None = no argument, and neither is the soft result
    plain = [t.clone() for t in infer.Predictor(det, CFG)(imgs, info)]
    none = infer.Predictor(det, CFG, soft_nms=None)(imgs, info)
    for a, b in zip(none, plain):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert torch.equal(plain[0], out[0]) and not torch.equal(plain[2], out[2])


def test_capacity_violations_are_refused_before_any_launch(cuda):
    from scda_amd import native as N
    lib, cap = N.lib(), N.soft_nms_capacity()
    boxes = torch.from_numpy(sc.make(64, False, False)).to(cuda)
    before = boxes.clone()
    seg = torch.tensor([[0, 64, 0]], dtype=torch.int64, device=cuda)
    keep = torch.full((64,), -7, dtype=torch.int64, device=cuda)
    num = torch.full((1,), -7, dtype=torch.int64, device=cuda)
    for S, max_n, method in ((1, cap + 1, 1), (1, 64, 3), (1, 64, -1), (0, 64, 1), (-1, 64, 1)):
        st = lib.scda_soft_nms_segments_hip(N._p(boxes), N._p(seg), S, max_n, method, 0.5, 0.3, 0.001, N._p(keep), N._p(num), N._stream())
        assert st == -1, (S, max_n, method)                             # SCDA_EINVAL
    with pytest.raises(N.ScdaNativeError, match="scda_soft_nms_segments_hip"):
        N.soft_nms_segments(boxes, seg, cap + 1, 1, 0.5, 0.3, 0.001)
    torch.cuda.synchronize()
    assert torch.equal(boxes, before) and (keep == -7).all() and (num == -7).all()
    # box prediction: P above the capacity
    B, P, C, top_n = 1, cap + 1, 2, 4
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=cuda)      # noqa: E731
    det, dc = torch.full((B, top_n, 7), -7.0, device=cuda), torch.full((B,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty(N.box_predict_workspace_bytes(B, P, C), dtype=torch.uint8, device=cuda)
    import ctypes
    s4, m4 = (ctypes.c_double * 4)(0.1, 0.1, 0.2, 0.2), (ctypes.c_double * 4)(0, 0, 0, 0)
    rois, counts, prob, loc, info = z(P, 5), z(B, dt=torch.int32), z(P, C), z(P, 4 * C), torch.tensor([[200., 312., 1.]], device=cuda)
    for p_, method in ((P, 1), (64, 3)):
        st = lib.scda_box_predict_soft_hip(N._p(rois), N._p(counts), B, p_, N._p(prob), N._p(loc), C, N._p(info), 3, s4, m4, 0.0, top_n,
                                           method, 0.5, 0.3, 0.001, N._p(ws), N._p(det), N._p(dc), N._stream())
        assert st == -1, (p_, method)
    torch.cuda.synchronize()
    assert (det == -7).all() and (dc == -7).all()
    # at the capacity itself the sweep runs: P = 2048 rows of one class in one image
    P = cap
    head = refs.synth_head(B=1, P=P, C=2, counts=(P,), empty_class=0, seed=9)
    det, dc = _box_predict(cuda, head, dict(CFG["test_predict_bbox_cfg"], score_thresh=0.0), refs.SETTINGS[1], 20)
    assert dc[0] == 20 and (np.diff(det[0, :, 5]) <= 0).all()
