"""The box kernels between the networks -- detection_ops.hip's NMS mask and sweep, infer_ops.hip, box_ops.hip -- on the MI355X at their
structural edges, against the plain numpy restatements of tests/box_refs.py (pinned on the CPU by tests/test_box_refs.py).

Everything here is BIT-EXACT: every expected value is an integer, a copied float or the result of single IEEE operations (float32 /
float64 + - * / and comparisons, compiled with -ffp-contract=off).  No tolerance appears in this file.  The two non-IEEE operations of
these kernels are kept out of the comparison by construction where that is possible: every size delta is 0 (exp(0) = 1 in every
libm, 0 * std + 0 = 0).  One known dependency remains: anchor_finalize's float64 log of gt width / anchor width is compared with
numpy's float64 log after BOTH are rounded to float32.  Two float64 logs that differ in their last bit give different float32
values only if the result lies within 2**-29 (relative) of a float32 rounding boundary; the inputs are fixed, so the comparison is
deterministic for a given libm and ROCm, and the existing golden tests hold 30720-anchor maps to the reference bit for bit on the
same grounds.  A libm or ROCm update could in principle flip such a bit: a failure confined to loc_targets' log columns (2, 3 of an
anchor) after such an update is that dependency, not the box logic."""
import functools

import numpy as np
import pytest
import torch

import box_refs as R
from test_host_functions import CFG
from test_infer_rules import proposals_by_rule

pytestmark = pytest.mark.gpu

F = np.float32
BAND, SENT = 64, -7            # sentinel band behind every buffer the test owns


def dev(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(cuda).contiguous()


def banded(n, dtype, cuda):
    """a buffer of n elements the kernel may write, with BAND sentinel elements behind it (and sentinels in it)"""
    return torch.full((n + BAND,), SENT, dtype=dtype, device=cuda)


def band_intact(t, n):
    return bool((t[n:] == SENT).all())


# ================================================================================================================ NMS ==========
def _nms_valid(cuda, boxes, valid, thresh, max_keep=0):
    """scda_nms_valid_hip on buffers the test owns -> keep list; nothing beyond the count may be written"""
    from scda_amd import native as N
    n = boxes.shape[0]
    d = dev(boxes, cuda) if n else torch.zeros(0, 5, device=cuda)
    keep, num = banded(n, torch.int64, cuda), banded(1, torch.int64, cuda)
    ws = torch.empty(max(N.lib().scda_nms_workspace_bytes(n), 8), dtype=torch.uint8, device=cuda)
    v = None if valid is None else dev(np.asarray(valid).astype(np.uint8), cuda)
    N._check(N.lib().scda_nms_valid_hip(N._p(d), N._p(v), n, thresh, N._p(ws), N._p(keep), N._p(num), max_keep, N._stream()), "scda_nms_valid_hip")
    k = int(num[0])
    assert 0 <= k <= n and band_intact(num, 1)
    assert bool((keep[k:] == SENT).all()), "the sweep wrote past its count"
    return keep[:k].cpu().numpy()


def _nms(cuda, boxes, thresh, max_keep=0):
    from scda_amd import native as N
    keep, num = N.nms(dev(boxes, cuda), thresh, max_keep=max_keep)
    return keep[:int(num)].cpu().numpy()


STRUCTURED = R.nms_structured_cases()


@functools.lru_cache(maxsize=None)
def _greedy(name):
    _, b, thresh = next(c for c in STRUCTURED if c[0] == name)
    return R.nms_greedy(b, thresh)


@pytest.mark.parametrize("name", [c[0] for c in STRUCTURED])
def test_nms_structured_lists(cuda, name):
    """chains across chunk and group-of-4 boundaries (box i suppresses only i + 1: the 64-chain needs 64 fixpoint rounds of the 66
    allowed), two-step chains, one box suppressing all, nothing overlapping, pairs whose IoU is exactly the threshold (strict >:
    the later box is kept)"""
    _, b, thresh = next(c for c in STRUCTURED if c[0] == name)
    want = _greedy(name)
    np.testing.assert_array_equal(_nms(cuda, b, thresh), want)
    np.testing.assert_array_equal(_nms_valid(cuda, b, None, thresh), want)
    np.testing.assert_array_equal(_nms_valid(cuda, b, np.ones(b.shape[0], bool), thresh), want)
    if name.startswith("chain_"):
        np.testing.assert_array_equal(want, np.arange(0, b.shape[0], 2))


# the chain of 513: 257 kept in all, 32 in chunk 0, 128 in group 0 (4 chunks)
@pytest.mark.parametrize("max_keep", [1, 31, 32, 33, 127, 128, 129, 256, 257, 258])
def test_nms_max_keep_on_chunk_and_group_ends(cuda, max_keep):
    b = R.chain_boxes(513)
    want = np.arange(0, 513, 2)[:max_keep]
    np.testing.assert_array_equal(R.nms_greedy(b, 0.5, max_keep=max_keep), want)
    np.testing.assert_array_equal(_nms(cuda, b, 0.5, max_keep), want)
    np.testing.assert_array_equal(_nms_valid(cuda, b, None, 0.5, max_keep), want)
    odd = np.arange(513) % 2 == 1                      # with the kept boxes invalidated the odd ones are kept: same ends, shifted by one
    np.testing.assert_array_equal(_nms_valid(cuda, b, odd, 0.5, max_keep), np.arange(1, 513, 2)[:max_keep])


@pytest.mark.parametrize("n", [200, 257])
@pytest.mark.parametrize("flags", ["none_valid", "last_only", "kept_invalidated", "valid_tail", "random"])
def test_nms_validity_flags(cuda, n, flags):
    b = R.chain_boxes(n)
    valid = {"none_valid": np.zeros(n, bool), "last_only": np.arange(n) == n - 1, "kept_invalidated": np.arange(n) % 2 == 1,
             "valid_tail": np.arange(n) >= 150, "random": np.random.RandomState(n).uniform(size=n) > 0.4}[flags]
    want = R.nms_greedy(b, 0.5, valid=valid)
    assert flags != "none_valid" or want.size == 0
    assert flags != "last_only" or list(want) == [n - 1]
    assert flags != "kept_invalidated" or list(want) == list(range(1, n, 2))
    np.testing.assert_array_equal(_nms_valid(cuda, b, valid, 0.5), want)
    np.testing.assert_array_equal(_nms_valid(cuda, b, valid, 0.5, 5), R.nms_greedy(b, 0.5, valid=valid, max_keep=5))


def test_nms_empty_list(cuda):
    assert _nms_valid(cuda, np.zeros((0, 5), F), None, 0.5).size == 0


def test_nms_segments_of_structured_lists(cuda):
    """lists of lengths 0, 1, 64, 65, 256, 257 mixing chains and disjoint boxes in ONE launch: each equals nms_greedy on it alone, through
    the wrapper and through the C entry on a sentinel-filled keep buffer: no slot past a list's count is written, so no list touches the
    next list's rows"""
    from scda_amd import native as N
    lists, thresh = R.segment_lists()
    boxes, seg, max_n = R.segment_table(lists)
    S, rows = seg.shape[0], boxes.shape[0]
    d, sg = dev(boxes, cuda), dev(seg, cuda)
    keep, num = N.nms_segments(d, sg, max_n, thresh)
    keep, num = keep.cpu().numpy(), num.cpu().numpy()
    own_keep, own_num = banded(rows, torch.int64, cuda), banded(S, torch.int64, cuda)
    words = int(seg[-1, 2] + seg[-1, 1] * ((seg[-1, 1] + 63) // 64))               # the lists' mask words, back to back
    ws = torch.empty(words + BAND, dtype=torch.int64, device=cuda)
    N._check(N.lib().scda_nms_segments_hip(N._p(d), N._p(sg), S, max_n, thresh, N._p(ws), N._p(own_keep), N._p(own_num), N._stream()),
             "scda_nms_segments_hip")
    torch.cuda.synchronize()
    assert band_intact(own_keep, rows) and band_intact(own_num, S)
    own_keep, own_num = own_keep[:rows].cpu().numpy(), own_num[:S].cpu().numpy()
    for s, b in enumerate(lists):
        want = R.nms_greedy(b, thresh)
        row, n = int(seg[s, 0]), int(seg[s, 1])
        assert num[s] == want.size and own_num[s] == want.size, s
        np.testing.assert_array_equal(keep[row:row + want.size], want, err_msg="list %d" % s)
        np.testing.assert_array_equal(own_keep[row:row + want.size], want, err_msg="list %d" % s)
        assert (own_keep[row + want.size:row + n] == SENT).all(), "list %d wrote past its count" % s


def test_nms_mask_upper_triangle_of_a_chain(cuda):
    from scda_amd import native as N
    for b, thresh in ((R.chain_boxes(257), 0.5), (R.exact_threshold_pairs(65, 1, 0.5), 0.5), (R.exact_threshold_pairs(65, 1, 0.7), 0.7)):
        n = b.shape[0]
        m = N.nms_mask(dev(b, cuda), thresh).cpu().numpy().view(np.uint64)
        want = R.nms_mask_np(b, thresh)
        upper = np.arange(want.shape[1])[None, :] >= (np.arange(n) // 64)[:, None]
        np.testing.assert_array_equal(m[upper], want[upper])


# =========================================================================================================== rpn_topk ==========
TOPK = ([(15, 21, 21, 1, t) for t in (6144, 6145, 6614, 6500)] + [(15, 21, 21, 3, 6145)] +        # KA 6615: select + LDS | workspace
        [(3, 1, 5, 1, t) for t in (1, 14, 15, 0)] + [(3, 1, 5, 2, 14)] +                          # KA 15 < one wave
        [(15, 3, 5, 1, t) for t in (1, 64, 224)])                                                 # KA 225 < 1024 threads


@pytest.mark.parametrize("kind", ["random", "quant3", "equal", "zero_one"])
@pytest.mark.parametrize("A,fh,fw,B,top_n", TOPK)
def test_rpn_topk_edges(cuda, A, fh, fw, B, top_n, kind):
    """select x workspace (6144 < n < KA), per-image key offsets on that path, n = 1, n = KA - 1, n = 6144 | 6145, KA below a wave / the
    workgroup, all-equal and 3-level score planes, exact 0.0 and 1.0: order == np.argsort(-s, kind='stable')[:n]; the bg channels
    hold NaN"""
    from scda_amd import native as N
    KA = A * fh * fw
    s = np.stack([R.score_plane(kind, KA, 1000 * b + KA + top_n) for b in range(B)])
    n = KA if top_n <= 0 or top_n >= KA else top_n
    want = np.stack([np.argsort(-s[b], kind='stable')[:n] for b in range(B)]).astype(np.int32)
    if kind == "equal":
        np.testing.assert_array_equal(want[0], np.arange(n))
    order = banded(B * n, torch.int32, cuda)
    got = N.rpn_topk(dev(R.prob_from_scores(s, A, fh, fw), cuda), top_n, order=order[:B * n].view(B, n))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert band_intact(order, B * n)


# ============================================================================================== rpn_proposals_batched ==========
def _rpn_outputs(B, A, fh, fw, seed):
    """soft-maxed scores [B,2A,fh,fw] and deltas [B,4A,fh,fw] whose size deltas are 0"""
    g = torch.Generator().manual_seed(seed)
    prob = torch.softmax(torch.randn(B, fh, fw, A, 2, generator=g) * 2.0, -1).reshape(B, fh, fw, 2 * A).permute(0, 3, 1, 2).contiguous()
    loc = torch.randn(B, fh, fw, A, 4, generator=g) * 0.3
    loc[..., 2:] = 0
    return prob, loc.reshape(B, fh, fw, 4 * A).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("pre,P,info", [(6145, 50, [[336, 336, 1], [1, 1, 1]]), (6145, 50, [[1, 1, 1], [300, 336, 1]]),
                                        (64, 100, [[336, 336, 1], [200, 250, 1]])])
def test_rpn_proposals_batched_edges(cuda, pre, P, info):
    """B = 2 at (21, 21): pre_nms_top_n 6145 (select + workspace keys, per-image offsets), an image so small that clipping makes
    every box fail roi_min_size (count 0, every row (b,0,0,0,0)), P larger than what is kept (pre = 64): rows == proposals_by_rule bit
    for bit, padding rows (b, 0, 0, 0, 0) with score 0"""
    from scda_amd import device_boxes
    from scda_amd import native as N
    cfg = dict(CFG["test_rpn_proposal_cfg"], pre_nms_top_n=pre, post_nms_top_n=P)
    B, A, fh, fw = 2, 15, 21, 21
    prob, loc = _rpn_outputs(B, A, fh, fw, pre + P)
    info = np.array(info, dtype=F)
    want = proposals_by_rule(prob, loc, cfg, info)
    a64 = device_boxes.anchors_on_device(fh, fw, cfg, torch.device(cuda))[1]
    rois5, props6, counts = banded(B * P * 5, torch.float32, cuda), banded(B * P * 6, torch.float32, cuda), banded(B, torch.int32, cuda)
    ws = torch.empty(N.rpn_proposals_workspace_bytes(B, A, fh, fw, pre), dtype=torch.uint8, device=cuda)
    N.rpn_proposals_batched(prob.to(cuda), loc.to(cuda), a64, dev(info, cuda), pre, cfg['roi_min_size'], cfg['nms_iou_thresh'], P, ws,
                            rois5[:B * P * 5].view(B * P, 5), props6[:B * P * 6].view(B * P, 6), counts[:B])
    torch.cuda.synchronize()
    assert band_intact(rois5, B * P * 5) and band_intact(props6, B * P * 6) and band_intact(counts, B)
    r5, p6, cnt = rois5[:B * P * 5].view(B, P, 5).cpu().numpy(), props6[:B * P * 6].view(B, P, 6).cpu().numpy(), counts[:B].cpu().numpy()
    for b in range(B):
        w = want[want[:, 0] == b]
        assert cnt[b] == w.shape[0], b
        assert (info[b, 0] > 1) == (cnt[b] > 0) and (pre > 64 or cnt[b] < P)
        np.testing.assert_array_equal(p6[b, :cnt[b]], w)
        pad = np.zeros((P - cnt[b], 6), F)
        pad[:, 0] = b
        np.testing.assert_array_equal(p6[b, cnt[b]:], pad)
        np.testing.assert_array_equal(r5[b], p6[b, :, :5])


# ========================================================================================================= box_predict ==========
CASES = {"a": R.predict_case_a, "b": R.predict_case_b, "c": R.predict_case_c}


@functools.lru_cache(maxsize=None)
def _predict_case(which):
    return CASES[which]()


@functools.lru_cache(maxsize=None)
def _predict_want(which, score_thresh):
    """the restatement at a top_n that cuts nothing; a smaller top_n is its first rows"""
    c = _predict_case(which)
    return R.predict_np(c["rois"], c["roi_counts"], c["P"], c["prob"], c["loc"], c["info"], dict(R.PREDICT_CFG, score_thresh=score_thresh, top_n=7000))


@pytest.mark.parametrize("which,score_thresh,top_n", [("a", 0.0, 100), ("a", 0.0, 7000), ("b", 0.0, 100), ("b", 0.0, 7000)] +
                         [("c", t, n) for t in (0.0, R.LEVELS[0]) for n in (1, 10, 100)])
def test_box_predict_edges(cuda, which, score_thresh, top_n):
    """(a) C = 81, P = 80, B = 2: 6400 kept rows per image sort in box_topn_kernel's workspace; (b) C = 2, P = 6150: the workspace
    branch of box_decode_sort_kernel (and of the top-n sort), ties inside the class; (c) C = 9, P = 64, B = 3, roi_counts [64, 0, 17],
    per-image image_info, 4 score levels: ties inside classes and across classes AT the top_n cut, scores equal to score_thresh
    dropped, top_n beyond what is kept.  Rows >= roi_counts[b] hold NaN in rois, prob and loc.  det and counts == predict_np."""
    from scda_amd import native as N
    c = _predict_case(which)
    full, full_counts = _predict_want(which, score_thresh)
    B, P, C = len(c["roi_counts"]), c["P"], c["prob"].shape[1]
    want = np.zeros((B, top_n, 7), F)
    k = min(top_n, 7000)
    want[:, :k] = full[:, :k]
    want_counts = np.minimum(full_counts, top_n)
    det, dc = banded(B * top_n * 7, torch.float32, cuda), banded(B, torch.int32, cuda)
    ws = torch.empty(N.box_predict_workspace_bytes(B, P, C), dtype=torch.uint8, device=cuda)
    N.box_predict(dev(c["rois"], cuda), dev(c["roi_counts"], cuda), dev(c["prob"], cuda), dev(c["loc"], cuda), dev(c["info"], cuda),
                  R.PREDICT_CFG['bbox_normalize_stds'], R.PREDICT_CFG['bbox_normalize_means'], score_thresh, R.PREDICT_CFG['nms_iou_thresh'],
                  top_n, ws, det[:B * top_n * 7].view(B, top_n, 7), dc[:B])
    torch.cuda.synchronize()
    assert band_intact(det, B * top_n * 7) and band_intact(dc, B)
    np.testing.assert_array_equal(dc[:B].cpu().numpy(), want_counts)
    got = det[:B * top_n * 7].view(B, top_n, 7).cpu().numpy()
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(got, want)


# ============================================================================================================= box_ops ==========
def _anchor_bufs(KA, G, cuda):
    i32 = torch.int32
    return {"best_iou": banded(KA, torch.float32, cuda), "best_gt": banded(KA, i32, cuda), "gt_best": banded(G, i32, cuda),
            "labels": banded(KA, torch.int8, cuda), "pos_list": banded(KA, i32, cuda), "neg_list": banded(KA, i32, cuda),
            "counts": banded(2, i32, cuda)}


def _check_lists(bufs, L, n):
    """labels, best gt / IoU, the ordered lists and counts of anchor_label / proposal_match against the restatement; nothing is
    written behind a list's count or behind a buffer"""
    n_pos, n_neg = (int(v) for v in bufs["counts"][:2].cpu())
    assert [n_pos, n_neg] == list(L["counts"])
    np.testing.assert_array_equal(bufs["labels"][:n].cpu().numpy(), L["labels"])
    np.testing.assert_array_equal(bufs["best_gt"][:n].cpu().numpy(), L["best_gt"])
    np.testing.assert_array_equal(bufs["best_iou"][:n].cpu().numpy(), L["best_iou"])
    np.testing.assert_array_equal(bufs["pos_list"][:n_pos].cpu().numpy(), L["pos_list"])
    np.testing.assert_array_equal(bufs["neg_list"][:n_neg].cpu().numpy(), L["neg_list"])
    assert band_intact(bufs["pos_list"], n_pos) and band_intact(bufs["neg_list"], n_neg) and band_intact(bufs["counts"], 2)
    for k in ("labels", "best_gt", "best_iou"):
        assert band_intact(bufs[k], n), k


def _anchor_round_trip(cuda, anchors32, anchors64, gts, A, fh, fw, neg=0.3, pos=0.7, min_gt_best=0.1):
    """anchor_label, then anchor_finalize with drop lists that are empty (no pointer, and a zero-length tensor), hold one element, and
    cover the whole lists"""
    from scda_amd import native as N
    KA, G = anchors32.shape[0], gts.shape[0]
    assert KA == A * fh * fw
    L = R.anchor_labels_np(anchors32, gts, neg, pos, min_gt_best)
    a32, a64, g = dev(anchors32, cuda), dev(anchors64, cuda), dev(gts, cuda)
    n_pos, n_neg = (int(v) for v in L["counts"])
    drops = [(None, None), (np.zeros(0, np.int64), np.zeros(0, np.int64)), (np.arange(n_pos), np.arange(n_neg)[::-1].copy())]
    if n_pos and n_neg:
        drops.append((np.array([n_pos - 1]), np.array([0])))
    if n_pos > 2:
        drops.append((np.arange(0, n_pos, 2), None))
    for drop_pos, drop_neg in drops:
        bufs = _anchor_bufs(KA, G, cuda)
        N.anchor_label(a32, g, neg, pos, min_gt_best, bufs)
        torch.cuda.synchronize()
        _check_lists(bufs, L, KA)
        assert band_intact(bufs["gt_best"], G)
        per_gt = R.iou_f32(anchors32, gts).max(axis=0)
        np.testing.assert_array_equal(bufs["gt_best"][:G].cpu().numpy().view(F), per_gt)
        dp = None if drop_pos is None else dev(drop_pos.astype(np.int32), cuda)     # indices < the counts only; empty: no pointer, or a
        dn = None if drop_neg is None else dev(drop_neg.astype(np.int32), cuda)     # zero-length tensor
        cls_t, loc_t, loc_m = N.anchor_finalize(bufs, dp, dn, a64, g, A, fh, fw)
        labels = R.apply_drops(L["labels"], L["pos_list"], drop_pos, L["neg_list"], drop_neg)
        c2, t2, m2 = R.anchor_maps_np(labels, L["best_gt"], anchors64, gts, A, fh, fw)
        np.testing.assert_array_equal(bufs["labels"][:KA].cpu().numpy(), labels)
        np.testing.assert_array_equal(cls_t.cpu().numpy()[0], c2)
        np.testing.assert_array_equal(loc_t.cpu().numpy()[0], t2)
        np.testing.assert_array_equal(loc_m.cpu().numpy()[0], m2)
        assert band_intact(bufs["labels"], KA)
    return L


GRID_GTS = np.array([[20, 10, 110, 90, 3], [150, 40, 290, 180, 5], [8, 100, 60, 170, 1], [3, 3, 12, 12, 2], [60, 60, 61, 61, 4]], dtype=F)


@pytest.mark.parametrize("fh,fw", [(12, 19), (3, 5), (1, 1)])
def test_boxops_anchor_targets_on_small_grids(cuda, fh, fw):
    """KA = 3420 (no multiple of 256), 225 and 15 (< the 1024 threads of anchor_compact_kernel: lo > KA for most of them)"""
    from scda_amd.dropin.utils import anchor_helper
    cfg = CFG["train_anchor_target_cfg"]
    a = anchor_helper.get_anchors_over_plane(fh, fw, cfg['anchor_ratios'], cfg['anchor_scales'], cfg['anchor_stride'])
    L = _anchor_round_trip(cuda, a.astype(F), np.array(a), GRID_GTS, 15, fh, fw)
    assert L["counts"][0] > 0 and L["counts"][1] > 0


@pytest.mark.parametrize("KA,G,stride", [(1, 1, 5), (1, 2, 6), (255, 1, 5), (255, 2, 6), (257, 300, 5), (1023, 2, 5), (1023, 300, 6), (1025, 1, 6),
                                         (1025, 300, 5)])
def test_boxops_anchor_targets_on_custom_anchor_arrays(cuda, KA, G, stride):
    """arbitrary anchor arrays around the 256-thread block and the 1024-thread compaction, G = 300 (the strided LDS loops of
    anchor_match_kernel run twice), gt rows of stride 5 and 6 (NaN in the padding column), a duplicated gt (the claim goes to the
    LAST), integer boxes (IoU ties between gts)"""
    a, gts = R.random_anchor_case(KA, G, stride, KA + G)
    A, fh, fw = R.factor_KA(KA)
    _anchor_round_trip(cuda, a, a.astype(np.float64), gts, A, fh, fw)


@pytest.mark.parametrize("stride", [5, 6])
def test_boxops_anchor_labels_on_the_thresholds(cuda, stride):
    """IoU == 0.7f is not positive, IoU == 0.3f is not negative, a gt nobody reaches 0.1 on claims nothing, two identical gt rows: the
    last claims; then all positive / all negative / all ignore"""
    a, gts, want = R.threshold_anchor_case(stride)
    L = _anchor_round_trip(cuda, a, a.astype(np.float64), gts, 7, 1, 1)
    np.testing.assert_array_equal(L["labels"], want)
    assert L["best_gt"][3] == 2
    every = [(_anchor_round_trip(cuda, gts[:3, :4].copy(), gts[:3, :4].astype(np.float64), gts, 3, 1, 1), 1),
             (_anchor_round_trip(cuda, a[4:6].copy(), a[4:6].astype(np.float64), gts, 2, 1, 1), 0),
             (_anchor_round_trip(cuda, a[[0, 2, 6]].copy(), a[[0, 2, 6]].astype(np.float64), gts, 1, 1, 3, min_gt_best=0.95), -1)]
    for L, lab in every:
        assert (L["labels"] == lab).all()


@pytest.mark.parametrize("n_prop", [0, 1, 1023, 1024, 1025, 4097])
def test_boxops_proposal_match_edges(cuda, n_prop):
    """candidates around the 1024-thread compaction (per = 1 | 2 | 5 elements a thread, ragged last chunk), none at all (the gts
    alone), wholly outside the image, best_iou exactly on the thresholds: candidate 0 ON neg_lo (background) for n_prop >= 1, candidates 1
    and 2 ON pos and neg_hi (neither) for n_prop >= 3; _check_lists compares the device's labels of these rows with the restatement's"""
    from scda_amd import native as N
    props, gts = R.threshold_proposals(n_prop, n_prop + 1)
    M = R.proposal_match_np(props, gts, 200, 300, 0.7, 0.5, 0.1)
    n = n_prop + gts.shape[0]
    i32 = torch.int32
    bufs = {"rois": banded(n * 4, torch.float32, cuda), "best_iou": banded(n, torch.float32, cuda), "best_gt": banded(n, i32, cuda),
            "labels": banded(n, torch.int8, cuda), "pos_list": banded(n, i32, cuda), "neg_list": banded(n, i32, cuda), "counts": banded(2, i32, cuda)}
    p = dev(props, cuda) if n_prop else torch.zeros(0, 6, device=cuda)
    N.proposal_match(p, dev(gts, cuda), 200.0, 300.0, 0.7, 0.5, 0.1, bufs)
    torch.cuda.synchronize()
    _check_lists(bufs, M, n)
    np.testing.assert_array_equal(bufs["rois"][:n * 4].view(n, 4).cpu().numpy(), M["rois"])
    assert band_intact(bufs["rois"], n * 4)
    if n_prop >= 3:
        np.testing.assert_array_equal(M["labels"][:3], [0, -1, -1])


@pytest.mark.parametrize("rows,C", [(1, 2), (1, 81), (512, 2), (512, 81)])
@pytest.mark.parametrize("mix", ["all_background", "all_foreground", "mixed"])
def test_boxops_proposal_finalize_edges(cuda, rows, C, mix):
    from scda_amd import native as N
    rs = np.random.RandomState(rows + C)
    n_cand, G = 700, 6
    cand = rs.uniform(0, 300, (n_cand, 4)).astype(F)
    gts = np.zeros((G, 6), F)
    gts[:, :4] = rs.uniform(0, 300, (G, 4))
    gts[:, 4] = rs.randint(1, C, G)
    gts[0, 4], gts[1, 4] = 1, C - 1                              # the first and the last class column
    gts[:, 5] = np.nan
    sel = rs.randint(0, n_cand, rows).astype(np.int32)
    gt_of = {"all_background": np.full(rows, -1), "all_foreground": rs.randint(0, G, rows),
             "mixed": np.where(rs.uniform(size=rows) < 0.3, rs.randint(0, G, rows), -1)}[mix].astype(np.int32)
    enc = rs.uniform(-2, 2, (rows, 4)).astype(F)
    got = N.proposal_finalize(dev(cand, cuda), dev(sel, cuda), dev(gt_of, cuda), dev(enc, cuda), dev(gts, cuda), C, 3.0)
    want = R.proposal_finalize_np(cand, sel, gt_of, enc, gts, C, 3.0)
    for g, w in zip(got, want):
        assert g.dtype == torch.from_numpy(w).dtype
        np.testing.assert_array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("fh,fw,top_n,min_size,max_keep", [(3, 5, 225, 2, 0), (3, 5, 100, 2, 300), (3, 5, 100, 5000, 300), (12, 19, 0, 2, 40),
                                                          (1, 1, 15, 2, 4)])
def test_boxops_proposals_from_ranking_and_gather(cuda, fh, fw, top_n, min_size, max_keep):
    """decode + clip + size test + flagged NMS + gather of one image on ranked candidates (size deltas 0: the host's exponentials are
    ones): fewer kept than rows, none kept (no box passes the size test), more kept than rows; rows past the count stay untouched"""
    from scda_amd import native as N
    from scda_amd.dropin.utils import anchor_helper
    cfg = CFG["test_rpn_proposal_cfg"]
    A, KA = 15, 15 * fh * fw
    prob, loc = _rpn_outputs(1, A, fh, fw, KA + top_n)
    anchors = np.array(anchor_helper.get_anchors_over_plane(fh, fw, cfg['anchor_ratios'], cfg['anchor_scales'], cfg['anchor_stride']))
    score = prob.permute(0, 2, 3, 1).reshape(-1, 2)[:, 1].numpy()
    deltas = loc.permute(0, 2, 3, 1).reshape(-1, 4).numpy()
    order = R.topk_stable(score, top_n).astype(np.int32)
    n = order.size
    ones = np.ones((n, 2), F)
    img_h, img_w = fh * 16.0 - 3, fw * 16.0 - 5
    want = R.proposals_np(score, deltas, anchors, img_h, img_w, top_n, min_size, 0.7, max_keep, 2.0, order=order, exp_wh32=ones)
    a64, p, l = dev(anchors, cuda), prob[0].contiguous().to(cuda), loc[0].contiguous().to(cuda)
    out6, num = N.proposals_from_ranking(dev(order, cuda), dev(ones, cuda), a64, l, p, A, fh, fw, img_h, img_w, float(min_size), 0.7, max_keep, 2.0)
    k = int(num)
    assert k == want.shape[0] and (min_size < 5000 or k == 0)
    np.testing.assert_array_equal(out6[:k].cpu().numpy(), want)
    assert not out6[k:].any()                                        # (the wrapper's buffer starts as zeros)
    # the gather alone, on a buffer the test owns: num_keep 0 | < rows | > rows
    L = N.lib()
    props = dev(np.concatenate([R.decode_np(anchors[order], deltas[order], ones, img_h, img_w, min_size)[0], score[order][:, None]], 1), cuda)
    keep_all = R.nms_greedy(props.cpu().numpy(), 0.7)
    keep_dev = dev(keep_all, cuda)
    for num_keep, rows in ((0, 8), (min(3, keep_all.size), 8), (keep_all.size, max(1, keep_all.size - 2))):
        out = banded(rows * 6, torch.float32, cuda)
        num_dev = torch.tensor([num_keep], dtype=torch.int64, device=cuda)
        N._check(L.scda_proposal_gather_hip(N._p(props), N._p(keep_dev), N._p(num_dev), 5.0, rows, N._p(out), N._stream()),
                 "scda_proposal_gather_hip")
        torch.cuda.synchronize()
        w = min(num_keep, rows)
        np.testing.assert_array_equal(out[:w * 6].view(w, 6).cpu().numpy(),
                                      np.concatenate([np.full((w, 1), 5.0, F), props.cpu().numpy()[keep_all[:w]]], 1))
        assert band_intact(out, w * 6)
