"""tests/box_refs.py pinned on the CPU: every numpy restatement equals what already stands -- the C oracle, the reference's golden
vectors, this repository's numpy path (SCDA_DEVICE_BOXES=0) -- and every structured input has the property it is built for,
asserted rather than assumed.  tests/test_box_edges_gpu.py then holds the HIP kernels to these restatements bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

import box_refs as R
import nms_cases
from oracle import native_ops as orc
from test_host_functions import CFG, cpu_backend, synth_rpn_outputs  # noqa: F401  (cpu_backend: a fixture)
from test_infer_rules import assert_equal_up_to_tied_runs, predict_by_rule, rank_desc_later_first, rank_topk

F = np.float32
STRUCTURED = R.nms_structured_cases()
GRIDS = [(12, 19), (3, 5), (1, 1)]


@pytest.fixture(autouse=True)
def numpy_path(monkeypatch):
    monkeypatch.setenv("SCDA_DEVICE_BOXES", "0")


# ---------------------------------------------------------------------------------------------------------------- NMS ----------
@pytest.mark.parametrize("name", [c[0] for c in nms_cases.CASES if c[1] <= 2000])
def test_nms_greedy_equals_oracle_and_reference_keep_lists(golden_dir, name):
    g = np.load(os.path.join(golden_dir, "nms_ref.npz"))
    dets, thresh, keep = nms_cases.make(name), next(c[3] for c in nms_cases.CASES if c[0] == name), g[name + "_keep"].astype(np.int64)
    assert nms_cases.digest(dets) == str(g[name + "_sha256"])
    got = R.nms_greedy(dets, thresh)
    np.testing.assert_array_equal(got, keep)
    np.testing.assert_array_equal(got, orc.nms(dets, thresh))
    np.testing.assert_array_equal(R.nms_greedy(dets, thresh, max_keep=7), keep[:7])


@pytest.mark.parametrize("name", [c[0] for c in STRUCTURED])
def test_structured_nms_inputs_have_their_property(name):
    _, b, thresh = next(c for c in STRUCTURED if c[0] == name)
    n = b.shape[0]
    keep = R.nms_greedy(b, thresh)
    np.testing.assert_array_equal(keep, orc.nms(b, thresh))
    assert n < 2 or (np.diff(b[:, 4]) < 0).all()
    if name.startswith("chain_"):
        assert nms_cases.iou_rows_f32(b, 0, np.array([1]))[0] == F(0.6) and abs(nms_cases.iou_rows_f32(b, 0, np.array([2]))[0] - 1 / 3) < 1e-6
        np.testing.assert_array_equal(keep, np.arange(0, n, 2))
    elif name.startswith("chain2_at_threshold"):
        assert nms_cases.iou_rows_f32(b, 0, np.array([2]))[0] == F(0.5)          # ON the threshold: box i + 2 survives box i
        np.testing.assert_array_equal(keep, np.arange(0, n, 2))
    elif name.startswith("chain2_"):
        np.testing.assert_array_equal(keep, np.arange(0, n, 3))                  # box i suppresses i + 1 and i + 2
    elif name.startswith("first_suppresses_all"):
        np.testing.assert_array_equal(keep, [0])
    elif name.startswith("nothing_overlaps"):
        np.testing.assert_array_equal(keep, np.arange(n))
        assert not R.nms_mask_np(b, thresh).any()
    else:
        assert name.startswith("pairs_")
        lead = int(name[-1])
        for i in range(lead, n, 2):
            assert nms_cases.iou_rows_f32(b, i, np.array([i + 1]))[0] == F(thresh), i
        assert len(nms_cases.tie_pairs(b, thresh)) == 65
        np.testing.assert_array_equal(keep, np.arange(n))                        # strict >: the later box of every pair is kept
        assert lead == 0 or (63, 64) in nms_cases.tie_pairs(b, thresh)           # a pair across the chunk boundary


def _fixpoint_rounds(b, thresh):
    """rounds of K <- cand & ~OR{D[j] : j in K} from K = everything until K reproduces itself, on ONE chunk (n <= 64)"""
    n = b.shape[0]
    D = [set(np.arange(i + 1, n)[nms_cases.iou_rows_f32(b, i, np.arange(i + 1, n)) > F(thresh)]) if i + 1 < n else set() for i in range(n)]
    K, rounds = set(range(n)), 0
    while True:
        S = set().union(*[D[j] for j in K]) if K else set()
        Kn = set(range(n)) - S
        rounds += 1
        if Kn == K:
            return rounds, sorted(K)
        K = Kn


def test_chain_of_64_needs_64_fixpoint_rounds():
    """the sweep's cap is 66 rounds: the 64-chain needs 64 to settle (+ the one that sees it settled), random inputs 2 - 5"""
    rounds, K = _fixpoint_rounds(R.chain_boxes(64), 0.5)
    assert K == list(range(0, 64, 2))
    assert 64 <= rounds <= 66
    rounds, _ = _fixpoint_rounds(nms_cases.make("sparse_65_t07")[:64], 0.7)
    assert rounds <= 6


def test_nms_greedy_validity_and_max_keep():
    b = R.chain_boxes(200)
    rs = np.random.RandomState(2)
    for valid in (np.zeros(200, bool), np.arange(200) == 199, np.arange(200) % 2 == 1, np.arange(200) >= 150, rs.uniform(size=200) > 0.4):
        want = np.nonzero(valid)[0][orc.nms(b[valid], 0.5)] if valid.any() else np.zeros(0, np.int64)
        np.testing.assert_array_equal(R.nms_greedy(b, 0.5, valid=valid), want)
        np.testing.assert_array_equal(R.nms_greedy(b, 0.5, valid=valid, max_keep=9), want[:9])
    np.testing.assert_array_equal(R.nms_greedy(b, 0.5, valid=np.arange(200) % 2 == 1), np.arange(1, 200, 2))
    np.testing.assert_array_equal(R.nms_greedy(b, 0.5, valid=np.arange(200) >= 150), np.arange(150, 200, 2))


def test_nms_mask_np_equals_oracle_mask():
    for b, t in ((R.chain_boxes(257), 0.5), (nms_cases.make("rpn_300_t07"), 0.7), (R.exact_threshold_pairs(65, 1, 0.5), 0.5)):
        m, ref = R.nms_mask_np(b, t), orc.nms_mask(b, t)
        n, cb = ref.shape
        upper = np.arange(cb)[None, :] >= (np.arange(n) // 64)[:, None]
        np.testing.assert_array_equal(m[upper], ref[upper])


def test_segment_lists():
    lists, thresh = R.segment_lists()
    assert sorted(b.shape[0] for b in lists)[:7] == [0, 0, 1, 64, 64, 65, 65] and {256, 257} <= {b.shape[0] for b in lists}
    boxes, seg, max_n = R.segment_table(lists)
    assert max_n == 257 and boxes.shape[0] == seg[:, 1].sum()
    for b, (row, n, word) in zip(lists, seg):
        np.testing.assert_array_equal(boxes[row:row + n], b)
        np.testing.assert_array_equal(R.nms_greedy(b, thresh), orc.nms(b, thresh) if n else np.zeros(0, np.int64))
        assert n < 64 or 0 < len(R.nms_greedy(b, thresh)) <= n


# ----------------------------------------------------------------------------------------------------------- ranking ----------
def test_ranking_rules_and_score_planes():
    for kind in ("random", "quant3", "equal", "zero_one"):
        s = R.score_plane(kind, 225, 5)
        assert s.dtype == F and s.min() >= 0 and s.max() <= 1
        for top_n in (0, 1, 64, 224, 225, 300):
            np.testing.assert_array_equal(R.topk_stable(s, top_n), rank_topk(s, top_n))
        np.testing.assert_array_equal(R.rank_desc_later_first(s), rank_desc_later_first(s))
        p = torch.from_numpy(R.prob_from_scores(s[None], 15, 3, 5))
        np.testing.assert_array_equal(p.permute(0, 2, 3, 1).reshape(1, -1, 2)[0, :, 1].numpy(), s)   # the layout the kernel reads
        assert torch.isnan(p[:, 0::2]).all()
    assert len(np.unique(R.score_plane("quant3", 6615, 1))) == 3
    np.testing.assert_array_equal(R.topk_stable(R.score_plane("equal", 15, 1), 14), np.arange(14))
    z = R.score_plane("zero_one", 6615, 1)
    assert (z == 0).sum() > 100 and (z == 1).sum() > 100


# ----------------------------------------------------------------------------------------------------- box arithmetic ----------
def test_iou_f32_equals_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "bbox_overlaps.npz"))
    for case in ("small", "anchors", "degenerate"):
        np.testing.assert_array_equal(R.iou_f32(g[case + "_boxes"], g[case + "_query"]), g[case + "_out"], err_msg=case)
    for KA, G, stride in ((255, 2, 5), (1025, 300, 6)):
        a, gts = R.random_anchor_case(KA, G, stride, KA)
        np.testing.assert_array_equal(R.iou_f32(a, gts), orc.bbox_overlaps(a, gts[:, :4]))


def _anchor_targets_by_restatement(fh, fw, cfg, gts):
    from scda_amd.dropin.utils import anchor_helper
    anchors = anchor_helper.get_anchors_over_plane(fh, fw, cfg['anchor_ratios'], cfg['anchor_scales'], cfg['anchor_stride'])
    A = anchors.shape[0] // (fh * fw)
    L = R.anchor_labels_np(anchors.astype(F), gts, cfg['negative_iou_thresh'], cfg['positive_iou_thresh'], 0.1)
    n_pos, n_neg = (int(v) for v in L["counts"])
    budget = cfg['rpn_batch_size']
    max_pos = int(cfg['positive_percent'] * budget)
    drop_pos = drop_neg = None
    if n_pos > max_pos:                                                    # the reference's two draws (:66-80)
        drop_pos = np.random.choice(n_pos, size=n_pos - max_pos, replace=False)
        n_pos = max_pos
    if n_neg > budget - n_pos:
        drop_neg = np.random.choice(n_neg, size=n_neg - (budget - n_pos), replace=False)
        n_neg = budget - n_pos
    labels = R.apply_drops(L["labels"], L["pos_list"], drop_pos, L["neg_list"], drop_neg)
    return R.anchor_maps_np(labels, L["best_gt"], anchors, gts, A, fh, fw) + (max(1, n_pos + n_neg),)


GRID_GTS = np.array([[20, 10, 110, 90, 3], [150, 40, 290, 180, 5], [8, 100, 60, 170, 1], [3, 3, 12, 12, 2], [60, 60, 61, 61, 4]], dtype=F)


def _check_anchor_restatement(fh, fw, gts, seed):
    from scda_amd.dropin.functions.anchor_target import compute_anchor_targets
    cfg = CFG["train_anchor_target_cfg"]
    np.random.seed(seed)
    ct, lt, lm, norm = compute_anchor_targets((1, 60, fh, fw), cfg, torch.from_numpy(gts[None]), torch.tensor([[fh * 16, fw * 16, 1.0]]), None)
    after = np.random.rand()
    np.random.seed(seed)
    c2, l2, m2, n2 = _anchor_targets_by_restatement(fh, fw, cfg, gts)
    assert after == np.random.rand()
    np.testing.assert_array_equal(ct.numpy()[0], c2)
    np.testing.assert_array_equal(lt.numpy()[0], l2)
    np.testing.assert_array_equal(lm.numpy()[0], m2)
    assert norm == n2 and ct.dtype == torch.int64 and c2.dtype == np.int64 and l2.dtype == F


@pytest.mark.parametrize("G", [3, 12, 30])
def test_anchor_restatement_equals_numpy_path_on_fixtures(golden_dir, cpu_backend, G):
    g = np.load(os.path.join(golden_dir, "l2_G%d.npz" % G))
    _check_anchor_restatement(32, 64, g["gts"][0], int(g["seed"]))


@pytest.mark.parametrize("fh,fw", GRIDS)
def test_anchor_restatement_equals_numpy_path_on_grids(cpu_backend, fh, fw):
    _check_anchor_restatement(fh, fw, GRID_GTS, 3)


def _proposals_by_restatement(cls, loc, cfg, info):
    from scda_amd.dropin.utils import anchor_helper
    _, A4, fh, fw = loc.shape
    anchors = anchor_helper.get_anchors_over_plane(fh, fw, cfg['anchor_ratios'], cfg['anchor_scales'], cfg['anchor_stride'])
    score = cls.permute(0, 2, 3, 1).reshape(-1, 2)[:, 1].numpy()
    deltas = loc.permute(0, 2, 3, 1).reshape(-1, 4).numpy()
    return R.proposals_np(score, deltas, anchors, info[0][0], info[0][1], cfg['pre_nms_top_n'], cfg['roi_min_size'], cfg['nms_iou_thresh'],
                          cfg['post_nms_top_n'], 0)


@pytest.mark.parametrize("G", [3, 12, 30])
def test_proposal_restatement_equals_numpy_path_on_fixtures(golden_dir, cpu_backend, G):
    from scda_amd.dropin.functions.rpn_proposal import compute_rpn_proposals
    g = np.load(os.path.join(golden_dir, "l2_G%d.npz" % G))
    cls, loc = synth_rpn_outputs(int(g["seed"]))
    for key in ("test_rpn_proposal_cfg",) + (("train_rpn_proposal_cfg",) if G == 3 else ()):
        want = compute_rpn_proposals(cls, loc, CFG[key], g["image_info"]).numpy()
        assert_equal_up_to_tied_runs(_proposals_by_restatement(cls, loc, CFG[key], g["image_info"]), want, 5)


@pytest.mark.parametrize("fh,fw", GRIDS)
def test_proposal_restatement_equals_numpy_path_on_grids(cpu_backend, fh, fw):
    from scda_amd.dropin.functions.rpn_proposal import compute_rpn_proposals
    cls, loc = synth_rpn_outputs(9, fh=fh, fw=fw)
    info = np.array([[fh * 16, fw * 16, 1.0]], dtype=F)
    for pre, post, min_size in ((0, 300, 2), (100, 20, 2), (14, 300, 40)):
        cfg = dict(CFG["test_rpn_proposal_cfg"], pre_nms_top_n=pre, post_nms_top_n=post, roi_min_size=min_size)
        want = compute_rpn_proposals(cls, loc, cfg, info).numpy().reshape(-1, 6)
        np.testing.assert_array_equal(_proposals_by_restatement(cls, loc, cfg, info), want)


def _proposal_targets_by_restatement(props, cfg, gts, info):
    """functions/proposal_target.py with the matching and the gather restated; the draws and numpy's float32 log stay as they are"""
    from scda_amd.dropin.utils import bbox_helper
    gts = gts[(gts[:, 2] > gts[:, 0] + 1) & (gts[:, 3] > gts[:, 1] + 1)]
    M = R.proposal_match_np(props, gts, info[0], info[1], cfg['positive_iou_thresh'], cfg['negative_iou_thresh_hi'], cfg['negative_iou_thresh_lo'])
    pos_r = M["pos_list"].astype(np.int64)
    pos_g = M["best_gt"].astype(np.int64)[pos_r]
    neg_r = np.array(list(set(M["neg_list"].astype(np.int64)) - set(pos_r)))
    per_image, n_pos = cfg['batch_size'], len(pos_r)
    want_pos = int(cfg['positive_percent'] * per_image)
    if want_pos < n_pos:
        pick = np.random.choice(n_pos, size=want_pos, replace=False)
        pos_r, pos_g, n_pos = pos_r[pick], pos_g[pick], want_pos
    if per_image - n_pos < len(neg_r):
        neg_r = neg_r[np.random.choice(len(neg_r), size=per_image - n_pos, replace=False)]
    pos_r, pos_g, neg_r = list(pos_r), list(pos_g), list(neg_r)
    enc = bbox_helper.compute_loc_targets(M["rois"][pos_r], gts[pos_g])
    enc = (enc - np.array(cfg['bbox_normalize_means'])[None, :]) / np.array(cfg['bbox_normalize_stds'])[None, :]
    sel = np.array(pos_r + neg_r, dtype=np.int64)
    gt_of = np.concatenate([np.array(pos_g, dtype=np.int64), np.full(len(neg_r), -1, dtype=np.int64)])
    enc_all = np.zeros((len(sel), 4), dtype=F)
    enc_all[:len(pos_r)] = enc.astype(F)
    if len(sel) < per_image:
        again = np.random.choice(len(sel), size=per_image - len(sel), replace=True)
        sel, gt_of, enc_all = np.concatenate([sel, sel[again]]), np.concatenate([gt_of, gt_of[again]]), np.vstack([enc_all, enc_all[again]])
    return R.proposal_finalize_np(M["rois"], sel, gt_of, enc_all, gts, cfg['num_classes'], 0.0)


def _check_proposal_targets(props, gts, info, seed):
    from scda_amd.dropin.functions.proposal_target import compute_proposal_targets
    cfg = copy.deepcopy(CFG["train_proposal_target_cfg"])
    np.random.seed(seed)
    want = compute_proposal_targets(torch.from_numpy(props), cfg, torch.from_numpy(gts[None]), torch.from_numpy(info[None]), None)
    after = np.random.rand()
    np.random.seed(seed)
    got = _proposal_targets_by_restatement(props, cfg, gts, info)
    assert after == np.random.rand()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b.numpy())
    assert got[0].shape == (512, 5) and got[2].shape == (512, 36) and (got[1] > 0).any() and (got[1] == 0).any()


@pytest.mark.parametrize("G", [3, 12, 30])
def test_proposal_target_restatement_equals_numpy_path_on_fixtures(golden_dir, cpu_backend, G):
    g = np.load(os.path.join(golden_dir, "l2_G%d.npz" % G))
    _check_proposal_targets(g["proposals"], g["gts"][0], g["image_info"][0], int(g["seed"]) + 1)


@pytest.mark.parametrize("n_prop", [1, 1025])
def test_proposal_target_restatement_equals_numpy_path_on_threshold_proposals(cpu_backend, n_prop):
    props, gts = R.threshold_proposals(n_prop, n_prop)
    _check_proposal_targets(props, gts, np.array([200, 300, 1], dtype=F), 4)


def test_threshold_proposals_sit_on_the_thresholds():
    props, gts = R.threshold_proposals(1025, 1)
    M = R.proposal_match_np(props, gts, 200, 300, 0.7, 0.5, 0.1)
    np.testing.assert_array_equal(M["best_iou"][:3], [F(0.1), F(0.7), F(0.5)])
    np.testing.assert_array_equal(M["labels"][:7], [0, -1, -1, -1, -1, 1, 1])     # on lo: background; on pos / hi: neither; outside: IoU 0 < lo
    np.testing.assert_array_equal(M["best_iou"][3:5], [0, 0])
    assert (M["rois"][3] == 0).all() and M["rois"][4, 0] == 299 and M["rois"][4, 2] == 299
    np.testing.assert_array_equal(M["labels"][-3:], [1, 1, 1])                    # the appended gts match themselves
    np.testing.assert_array_equal(M["best_gt"][-3:], [0, 1, 2])
    assert {-1, 0, 1} == set(M["labels"].tolist()) and M["counts"][0] == M["pos_list"].size
    assert M["rois"].min() == 0 and M["rois"][:, 0::2].max() == 299 and M["rois"][:, 1::2].max() == 199
    Z = R.proposal_match_np(np.zeros((0, 6), F), gts, 200, 300, 0.7, 0.5, 0.1)     # no proposals: the gts alone
    np.testing.assert_array_equal(Z["pos_list"], [0, 1, 2])


def test_threshold_anchor_case_sits_on_every_rule():
    for stride in (5, 6):
        a, gts, want = R.threshold_anchor_case(stride)
        iou = R.iou_f32(a, gts)
        assert iou[0, 0] == F(0.7) and iou[2, 0] == F(0.3) and iou[3, 1] == iou[3, 2] == F(0.9) and iou[4, 3] == F(0.01) and iou[6, 1] == F(0.5)
        L = R.anchor_labels_np(a, gts, 0.3, 0.7, 0.1)
        np.testing.assert_array_equal(L["labels"], want)
        assert iou[3].argmax() == 1 and L["best_gt"][3] == 2                      # the LAST gt that claims the anchor wins
        np.testing.assert_array_equal(L["best_gt"], [0, 0, 0, 2, 3, 0, 1])
        np.testing.assert_array_equal(L["pos_list"], [1, 3])
        np.testing.assert_array_equal(L["neg_list"], [4, 5])
        # all positive / all negative / all ignore
        assert (R.anchor_labels_np(gts[:3, :4], gts[:3], 0.3, 0.7, 0.1)["labels"] == 1).all()
        assert (R.anchor_labels_np(a[4:6], gts, 0.3, 0.7, 0.1)["labels"] == 0).all()
        assert (R.anchor_labels_np(a[[0, 2, 6]], gts, 0.3, 0.7, 0.95)["labels"] == -1).all()


@pytest.mark.parametrize("KA,G,stride", [(1, 1, 5), (255, 2, 6), (257, 300, 5), (1023, 2, 5), (1025, 300, 6)])
def test_random_anchor_cases_reach_every_label_and_the_claim_rule(KA, G, stride):
    a, gts = R.random_anchor_case(KA, G, stride, KA + G)
    L = R.anchor_labels_np(a, gts, 0.3, 0.7, 0.1)
    if KA > 1:
        assert {-1, 0, 1} == set(L["labels"].tolist())
        first = R.iou_f32(a, gts).argmax(axis=1)
        assert (L["best_gt"] != first).any()                                      # a claim moved best_gt off the first maximum
    assert L["counts"][0] == (L["labels"] == 1).sum() and (np.diff(L["pos_list"]) > 0).all() and (np.diff(L["neg_list"]) > 0).all()
    A, fh, fw = R.factor_KA(KA)
    c, t, m = R.anchor_maps_np(L["labels"], L["best_gt"], a.astype(np.float64), gts, A, fh, fw)
    assert c.shape == (A, fh, fw) and t.shape == (4 * A, fh, fw) and m.sum() == 4 * L["counts"][0] and np.isfinite(t).all()


# ------------------------------------------------------------------------------------------------------ box prediction ----------
def test_predict_np_reproduces_reference_detections(golden_dir):
    g = np.load(os.path.join(golden_dir, "predict_bbox.npz"))
    cfg = CFG["test_predict_bbox_cfg"]
    n_rows = g["rois"].shape[0]
    assert (g["rois"][:, 0] == 0).all()
    det, counts = R.predict_np(g["rois"], [n_rows], n_rows, g["pred_cls"], g["pred_loc"], g["image_info"], cfg)
    assert counts[0] == g["bboxes"].shape[0]
    np.testing.assert_array_equal(det[0, :counts[0]], g["bboxes"])
    assert not det[0, counts[0]:].any()
    # fixed capacity: NaN rows behind the count change nothing
    pad = lambda a: np.vstack([a, np.full((7, a.shape[1]), np.nan, F)])
    det2, counts2 = R.predict_np(pad(g["rois"]), [n_rows], n_rows + 7, pad(g["pred_cls"]), pad(g["pred_loc"]), g["image_info"], cfg)
    np.testing.assert_array_equal(det2, det)
    np.testing.assert_array_equal(counts2, counts)


def _predict(case, score_thresh, top_n):
    return R.predict_np(case["rois"], case["roi_counts"], case["P"], case["prob"], case["loc"], case["info"],
                        dict(R.PREDICT_CFG, score_thresh=score_thresh, top_n=top_n))


def test_predict_np_equals_predict_by_rule_on_case_c():
    c = R.predict_case_c()
    real = np.concatenate([np.arange(b * 64, b * 64 + m) for b, m in enumerate(c["roi_counts"])])
    rois = c["rois"][real].copy()
    rois[rois[:, 0] == 2, 0] = 1                      # predict_by_rule numbers images by what it finds: close the gap of the empty one
    for thr in (0.0, R.LEVELS[0]):
        want = predict_by_rule(rois, c["prob"][real], c["loc"][real], c["info"][[0, 2]], dict(R.PREDICT_CFG, score_thresh=thr, top_n=10))
        det, counts = _predict(c, thr, 10)
        assert list(counts) == [10, 0, 10]
        got = np.vstack([det[0], det[2]])
        got[10:, 0] = 1
        np.testing.assert_array_equal(got, want)


def test_predict_cases_have_their_properties():
    a = R.predict_case_a()
    det, counts = _predict(a, 0.0, 7000)
    assert list(counts) == [6400, 6400] and 6400 > 6144                         # every (row, class) kept: the workspace sort
    assert not np.isnan(det).any() and not det[:, 6400:].any()
    assert (np.diff(det[0, :6400, 5]) == 0).any()                               # ties across classes
    for b in range(2):                                                          # the box of class c is RoI + that class's own shift
        assert len(np.unique(det[b, :6400, 1:5], axis=0)) == 6400
    b_ = R.predict_case_b()
    full, counts = _predict(b_, 0.0, 7000)
    assert counts[0] == 6150 > 6144
    s = full[0, :6150, 5]
    assert s[99] == s[100] and (np.diff(s) <= 0).all() and len(np.unique(s)) == 64          # ties inside the class, one AT the cut
    c = R.predict_case_c()
    assert np.isnan(c["prob"][64:128]).all() and np.isnan(c["rois"][128 + 17:]).all() and np.isnan(c["loc"][128 + 17:]).all()
    full, counts = _predict(c, 0.0, 1000)
    assert counts[1] == 0 and counts[0] > 100 and counts[2] > 10 and not np.isnan(full).any()
    for b, cuts in ((0, (1, 10, 100)), (2, (1, 10))):
        for cut in cuts:                                                        # a tie AT the cut, between rows of different classes
            run = full[b, :counts[b]][full[b, :counts[b], 5] == full[b, cut - 1, 5]]
            assert full[b, cut - 1, 5] == full[b, cut, 5] and len(np.unique(run[:, 6])) > 1, (b, cut)
    assert (np.diff(full[0, :counts[0], 6])[np.diff(full[0, :counts[0], 5]) == 0] != 0).any()
    on = (c["prob"][:64, 1:] == F(R.LEVELS[0])).sum()
    assert on > 50                                                              # scores ON the threshold exist ...
    thr, counts_t = _predict(c, R.LEVELS[0], 1000)
    assert counts_t[0] < counts[0] and (thr[0, :counts_t[0], 5] > F(R.LEVELS[0])).all()     # ... and every one is dropped
    assert (full[2, :counts[2], 1:5].max(0) <= [159, 119, 159, 119]).all() and (full[2, :counts[2], 3] == 159).any()   # image 2 clips
