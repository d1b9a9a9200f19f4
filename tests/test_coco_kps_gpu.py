"""Keypoint AP (OKS) and category-agnostic evaluation (useCats = 0, proposal AR) on the MI355X (scda_amd/csrc/coco_eval.hip:
scda_coco_oks_hip, scda_coco_kp_rows_hip, scda_coco_match_ign_hip, scda_coco_regroup_hip, scda_coco_prop_rows_hip) against the arrays
recorded from the reference's own cocoeval.py (tests/golden/coco_kps_ref.npz) and the numpy restatement (tests/coco_kps_np.py): the OKS
within the bound between two exp implementations, everything behind it bit for bit, the stats within the summation bound."""
import os

import numpy as np
import pytest
import torch

import coco_eval_np as cnp
import coco_kps_np as knp
from conftest import ROOT
from test_coco_kps_rules import KP_SETS, NOCAT_SETS, OKS_TOL, XYXY_SETS, evaluated, fixture, nocat_inputs, segm_fixture

pytestmark = pytest.mark.gpu

KP_CAPS = {'kp_rules': (32, 4), 'kp_random': (48, 6), 'kp_blocks': (320, 12)}     # (detection slots, GT slots) per image
NOCAT_CAPS = {'nocat_rules': (8, 4), 'nocat_props': (1024, 16), 'nocat_xyxy': (8, 4), 'nocat_segm': (32, 8)}
T = 10


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _kp_batch(images, idx, D, G, cuda):
    """the images idx as CocoEvaluator.add takes them; every unused keypoint slot, of detections and GTs, is poisoned with NaN"""
    B, Kp = len(idx), 17
    det = np.zeros((B, D, 7), np.float32); dc = np.zeros(B, np.int32); gc = np.zeros(B, np.int32)
    gb = np.zeros((B, G, 4), np.float64); ga = np.zeros((B, G), np.float64); gi = np.zeros((B, G), np.uint8); gk = np.zeros((B, G), np.int32)
    kp = np.full((B, D, Kp, 3), np.nan, np.float32); gkp = np.full((B, G, Kp, 3), np.nan, np.float64); gnk = np.zeros((B, G), np.int32)
    for b, i in enumerate(idx):
        im = images[i]
        d, g = len(im['dt_score']), len(im['gt_cat'])
        dc[b], gc[b] = d, g
        det[b, :, 0] = b
        det[b, :, 1:5] = np.nan                                              # the corners are not read
        det[b, :d, 5], det[b, :d, 6] = im['dt_score'], im['dt_cat']
        kp[b, :d], gkp[b, :g], gnk[b, :g] = im['dt_kps'], im['gt_kps'], im['gt_num_kps']
        gb[b, :g], ga[b, :g], gi[b, :g], gk[b, :g] = im['gt_xywh'], im['gt_area'], im['gt_iscrowd'], im['gt_cat']
    args = [_dev(np.asarray([images[i]['image_id'] for i in idx], np.int32), cuda)] + [_dev(a, cuda) for a in (det, dc, gb, ga, gi, gk, gc)]
    return args, {'keypoints': _dev(kp, cuda), 'gt_keypoints': _dev(gkp, cuda), 'gt_num_keypoints': _dev(gnk, cuda)}


def _kp_evaluator(name, cuda, max_images=None, debug=True, **kw):
    from scda_amd.coco_eval import CocoEvaluator
    images, K, params, _ = evaluated(name)
    D, G = KP_CAPS[name]
    return CocoEvaluator(K, 'keypoints', num_keypoints=17, max_images=len(images) if max_images is None else max_images, max_dets_per_image=D,
                         max_gts_per_image=G, device=cuda, debug=debug, **kw)


def _collect(ev, images, order):
    res = {k: v.cpu().numpy().copy() for k, v in ev.accumulate().items()}
    res['stats'] = ev.summarize()
    res['npig'] = ev.npig.cpu().numpy()
    slot = {i: s for s, i in enumerate(order)}
    pick = lambda t: np.concatenate([t[slot[i], :len(images[i]['dt_score'])] for i in range(len(images))])   # noqa: E731
    res['rank'], res['bits'] = pick(ev.rank.cpu().numpy()), pick(ev.bits.cpu().numpy().view(np.uint32))
    if ev.debug_match is not None:
        res['match'] = pick(ev.debug_match.cpu().numpy())
    return res


def _kp_run(name, cuda, order=None, batch=None, debug=True):
    images = evaluated(name)[0]
    order = list(range(len(images))) if order is None else list(order)
    batch = len(images) if batch is None else batch
    ev = _kp_evaluator(name, cuda, debug=debug)
    for s in range(0, len(order), batch):
        args, kw = _kp_batch(images, order[s:s + batch], ev.D, ev.G, cuda)
        ev.add(*args, **kw)
    return _collect(ev, images, order)


_RUNS = {}


def _default_kp_run(name, cuda):
    if name not in _RUNS:
        _RUNS[name] = _kp_run(name, cuda)
    return _RUNS[name]


def _bits(res):
    t = np.arange(T)
    return (res['bits'][:, :, None] >> t) & 1, (res['bits'][:, :, None] >> (16 + t)) & 1


def _note_oks_diff(name, text):
    """profiles/coco_kps_oks_diff.txt holds ONE line per set, replaced by each run: the same figures leave the file as it was"""
    path = os.path.join(ROOT, "profiles", "coco_kps_oks_diff.txt")
    try:
        lines = {}
        if os.path.exists(path):
            with open(path) as f:
                lines = dict(ln.rstrip("\n").split(": ", 1) for ln in f if ": " in ln)
        lines[name] = text
        with open(path, "w") as f:
            f.writelines("%s: %s\n" % (k, lines[k]) for k in sorted(lines))
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------------------------ keypoints
@pytest.mark.parametrize("name", KP_SETS)
def test_oks_kernel_against_the_recorded_oks(cuda, name):
    from scda_amd import native as N
    images, K, params, _ = evaluated(name)
    D, G = KP_CAPS[name]
    args, kw = _kp_batch(images, list(range(len(images))), D, G, cuda)
    ids, det, dc, gb, ga, gi, gk, gc = args
    sentinel = -7.0
    out = torch.full((len(images), G, D), sentinel, dtype=torch.float64, device=cuda)
    ign = torch.full((len(images), G), 9, dtype=torch.uint8, device=cuda)
    vars_ = _dev((params['sigmas'] * 2) ** 2, cuda)
    N.coco_oks(kw['keypoints'], dc, kw['gt_keypoints'], gb, ga, gc, vars_, out=out, gt_iscrowd=gi, gt_num_keypoints=kw['gt_num_keypoints'],
               gt_ignore=ign)
    got, flags = out.cpu().numpy(), ign.cpu().numpy()
    worst = 0.0
    for b, im in enumerate(images):
        g, d = im['oks_ref'].shape
        want, have = im['oks_ref'], got[b, :g, :d]
        exact = (want == 1.0) | (want == 0.0)
        assert np.array_equal(have[exact], want[exact]), (name, b)
        if want.size:
            worst = max(worst, float(np.abs(have - want).max()))
        pad = np.ones((G, D), bool)
        pad[:g, :d] = False
        assert (got[b][pad] == sentinel).all(), (name, b)                     # NaN padding reached nothing, nothing else was written
        assert np.array_equal(flags[b, :g], im['gt_ignore']) and (flags[b, g:] == 9).all()
    print(name, "max |oks - reference|", worst)
    _note_oks_diff(name, "max |scda_coco_oks_hip - computeOks| = %.3e over %d pairs" % (worst, sum(im['oks_ref'].size for im in images)))
    assert worst <= OKS_TOL


@pytest.mark.parametrize("name", KP_SETS)
def test_keypoint_evaluator_equals_the_recorded_eval(cuda, name):
    z = fixture()
    got = _default_kp_run(name, cuda)
    part = z[name + '_rank'] >= 0
    assert np.array_equal(got['rank'][part], z[name + '_rank'][part]) and (got['rank'][~part] >= 20).all()
    assert np.array_equal(got['match'], z[name + '_match'])
    matched, ignored = _bits(got)
    assert np.array_equal(matched, (z[name + '_match'] >= 0).astype(np.uint32))
    assert np.array_equal(ignored, z[name + '_ignore'].astype(np.uint32))
    assert np.array_equal(got['npig'], z[name + '_npig'])
    for key in ('precision', 'recall', 'scores'):
        assert got[key].dtype == np.float64 and got[key].shape == z[name + '_' + key].shape
        assert np.array_equal(got[key], z[name + '_' + key]), (key, int((got[key] != z[name + '_' + key]).sum()))
    n = cnp.stat_counts(z[name + '_precision'], z[name + '_recall'], evaluated(name)[3]['specs'])
    print(name, "stats", got['stats'], "max |diff|", np.abs(got['stats'] - z[name + '_stats']).max())
    assert got['stats'].shape == (10,)
    assert np.all(np.abs(got['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53), (got['stats'], z[name + '_stats'])


@pytest.mark.parametrize("name", KP_SETS)
def test_keypoint_order_and_batching_do_not_matter(cuda, name):
    n = len(evaluated(name)[0])
    base = _default_kp_run(name, cuda)
    rev = list(range(n))[::-1]
    for r in (_kp_run(name, cuda, order=rev, batch=1, debug=False), _kp_run(name, cuda, order=rev, batch=3, debug=False),
              _kp_run(name, cuda, order=rev, debug=False)):
        for key in ('precision', 'recall', 'scores', 'stats', 'npig', 'rank', 'bits'):
            assert r[key].tobytes() == base[key].tobytes(), key


def test_a_max_dets_list_without_20_gives_minus_one(cuda):
    images = evaluated('kp_rules')[0]
    ev = _kp_evaluator('kp_rules', cuda, debug=False, params={'max_dets': [10, 100]})
    args, kw = _kp_batch(images, list(range(len(images))), ev.D, ev.G, cuda)
    ev.add(*args, **kw)
    assert ev.summarize().tolist() == [-1.0] * 10


# --------------------------------------------------------------------------------------------------------------- useCats = 0
def _prop_batch(images, idx, P, G, cuda):
    from test_coco_eval_gpu import _batch
    args, _ = _batch(images, idx, P, G, cuda)
    det = args[1].cpu().numpy()
    prop = np.ascontiguousarray(det[:, :, :6])                               # (b, x1, y1, x2, y2, score)
    return [args[0], _dev(prop, cuda)] + args[2:]


def _nocat_run(name, cuda, order=None, batch=None, xyxy_as_xywh=None, max_images=None):
    """a useCats = 0 set through a CocoEvaluator -> (host arrays with the per-detection ones back in the order GIVEN, perm_dets and
    perm_gts per image cut to the live places, the evaluator)"""
    from scda_amd.coco_eval import CocoEvaluator
    from test_coco_eval_gpu import _batch
    images, K, params = nocat_inputs(name)
    D, G = NOCAT_CAPS[name]
    segm = name == 'nocat_segm'
    order = list(range(len(images))) if order is None else list(order)
    batch = len(order) if batch is None else batch
    ev = CocoEvaluator(K, 'segm' if segm else 'bbox', max_images=len(images) if max_images is None else max_images, max_dets_per_image=D,
                       max_gts_per_image=G, device=cuda, params={'area_rng': params['area_rng'], 'max_dets': params['max_dets']},
                       debug=True, use_cats=False)
    for s in range(0, len(order), batch):
        if xyxy_as_xywh is None:
            args, kw = _batch(images, order[s:s + batch], D, G, cuda, segm_fixture() if segm else None, 'random_segm' if segm else None)
            ev.add(*args, **kw)
        else:
            ev.add_proposals(*_prop_batch(images, order[s:s + batch], D, G, cuda), xyxy_as_xywh=xyxy_as_xywh)
    return _nocat_collect(ev, images, order)


def _nocat_collect(ev, images, order):
    res = {k: v.cpu().numpy().copy() for k, v in ev.accumulate().items()}
    res['stats'] = ev.summarize()
    res['npig'] = ev.npig.cpu().numpy()
    A = ev.A
    rank_d, bits_d, match_d = ev.rank.cpu().numpy(), ev.bits.cpu().numpy().view(np.uint32), ev.debug_match.cpu().numpy()
    pds, pgs = ev.perm_dets.cpu().numpy(), ev.perm_gts.cpu().numpy()
    slot = {i: s for s, i in enumerate(order)}
    rank, bits, match, perm_d, perm_g = [], [], [], [], []
    for i in sorted(slot):
        s, im = slot[i], images[i]
        n = len(im['dt_score'])
        pd, pg = pds[s][pds[s] >= 0], pgs[s][pgs[s] >= 0]
        assert (pds[s][:len(pd)] >= 0).all() and (pgs[s][:len(pg)] >= 0).all()            # the live places come first
        r, b, m = np.full(n, -1, np.int32), np.zeros((n, A), np.uint32), np.full((n, A, T), -1, np.int32)
        r[pd], b[pd] = rank_d[s, :len(pd)], bits_d[s, :len(pd)]
        md = match_d[s, :len(pd)]
        m[pd] = np.where(md >= 0, pg[np.maximum(md, 0)] if len(pg) else -1, -1)
        rank.append(r); bits.append(b); match.append(m); perm_d.append(pd); perm_g.append(pg)
    res.update(rank=np.concatenate(rank), bits=np.concatenate(bits), match=np.concatenate(match), perm_d=perm_d, perm_g=perm_g)
    return res, ev


def _check_nocat(got, want_rank, want_match, want_ignore, max_det):
    part = want_rank >= 0
    assert np.array_equal(got['rank'][part], want_rank[part])
    assert ((got['rank'][~part] >= max_det) | (got['rank'][~part] == -1)).all()
    assert np.array_equal(got['match'], want_match)
    matched, ignored = _bits(got)
    assert np.array_equal(matched, (want_match >= 0).astype(np.uint32))
    assert np.array_equal(ignored, np.asarray(want_ignore).astype(np.uint32))


@pytest.mark.parametrize("name", NOCAT_SETS)
def test_use_cats_false_equals_the_recorded_eval(cuda, name):
    """class rows through add() ('bbox' and 'segm'), proposals through add_proposals(xyxy_as_xywh=True): the reference's 'proposal' run"""
    z = fixture()
    got, ev = _nocat_run(name, cuda, xyxy_as_xywh=True if name in XYXY_SETS else None)
    assert np.array_equal(np.concatenate(got['perm_d']), z[name + '_dt_order'])
    assert np.array_equal(np.concatenate(got['perm_g']), z[name + '_gt_order'])
    assert [len(p) for p in got['perm_d']] == z[name + '_dt_live'].tolist() and [len(p) for p in got['perm_g']] == z[name + '_gt_live'].tolist()
    _check_nocat(got, z[name + '_rank'], z[name + '_match'], z[name + '_ignore'], ev.max_dets[-1])
    assert np.array_equal(got['npig'], z[name + '_npig']) and got['npig'].shape[0] == 1
    for key in ('precision', 'recall', 'scores'):
        assert got[key].shape == z[name + '_' + key].shape and np.array_equal(got[key], z[name + '_' + key]), key
    specs = cnp.stat_specs(ev.iou_thrs, ev.max_dets)
    n = cnp.stat_counts(z[name + '_precision'], z[name + '_recall'], specs)
    print(name, "stats", got['stats'])
    assert got['stats'].shape == (12,) and np.all(np.abs(got['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53)


def test_proposals_with_true_widths_equal_the_restatement(cuda):
    """add_proposals' default: w = (double) x2 - (double) x1, against tests/coco_kps_np.py over the same rows; reversed, in batches of 1"""
    images, K, params = knp.load_box_set(fixture(), 'nocat_props', xyxy_as_xywh=False)
    want = knp.evaluate(images, K, params, use_cats=False)
    from test_coco_kps_rules import given_order
    for kw in ({}, {'order': [3, 2, 1, 0], 'batch': 1}):
        got, ev = _nocat_run('nocat_props', cuda, xyxy_as_xywh=False, **kw)
        w_rank, w_match, w_ignore = given_order('nocat_props', want, images)
        assert (w_rank >= 0).all() and np.array_equal(got['rank'], w_rank)    # every proposal is live and ranked, past the cut too
        _check_nocat(got, np.where(w_rank < 1000, w_rank, -1), w_match, w_ignore, 1000)
        for key in ('precision', 'recall', 'scores'):
            assert np.array_equal(got[key], want[key]), key
        n = cnp.stat_counts(want['precision'], want['recall'], want['specs'])
        assert np.all(np.abs(got['stats'] - want['stats']) <= 2.0 * n * 2.0 ** -53) and got['stats'][8] > 0, got['stats']


def test_coco_stats_over_proposals(cuda):
    """a seeded detector's RPN proposals through evaluate.coco_stats(proposals=True), ground truth cut from its own proposals, against
    the numpy restatement fed the downloaded proposals"""
    from scda_amd import evaluate, infer
    from scda_amd.coco_eval import CocoEvaluator
    from test_mask_infer_gpu import H_IMG, W_IMG, _images, _mask_detector
    det, cfg = _mask_detector(cuda, with_mask=False)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.0], [H_IMG, W_IMG, 1.0]])
    pred = infer.Predictor(det, cfg)
    out = pred(x, info)
    props, counts = out[0].cpu().numpy().copy(), out[1].cpu().numpy().copy()
    P, G = props.shape[1], 6
    assert counts.min() > 0 and P <= 1024
    gb = np.zeros((2, G, 4)); ga = np.zeros((2, G)); gi = np.zeros((2, G), np.uint8); gk = np.zeros((2, G), np.int32); gc = np.zeros(2, np.int32)
    for b in range(2):
        src = list(range(0, int(counts[b]), max(1, int(counts[b]) // G)))[:G]
        gc[b] = len(src)
        for g, j in enumerate(src):
            x1, y1, x2, y2 = props[b, j, 1:5].astype(np.float64)
            gb[b, g] = (x1 - 1, y1, x2 - x1 + 1, y2 - y1 + 2)
            ga[b, g], gi[b, g], gk[b, g] = gb[b, g, 2] * gb[b, g, 3], g == 1, 1 + g % 2
    item = {'image': x, 'image_info': info, 'image_ids': torch.tensor([12, 5], dtype=torch.int32), 'gt_boxes': _dev(gb, cuda),
            'gt_areas': _dev(ga, cuda), 'gt_iscrowd': _dev(gi, cuda), 'gt_categories': _dev(gk, cuda), 'gt_counts': _dev(gc, cuda)}
    new = lambda **kw: CocoEvaluator(2, 'bbox', max_images=2, max_dets_per_image=P, max_gts_per_image=G, device=cuda,     # noqa: E731
                                     params={'max_dets': [1, 100, 1000]}, **kw)
    stats = evaluate.coco_stats([item], pred, new(use_cats=False), proposals=True)
    images = []
    for b in range(2):
        n, g = int(counts[b]), int(gc[b])
        xywh = cnp.xywh_from_corners(props[b, :n, 1:5])
        images.append({'image_id': [12, 5][b], 'dt_xywh': xywh, 'dt_score': props[b, :n, 5], 'dt_cat': np.ones(n, np.int32),
                       'dt_area': xywh[:, 2] * xywh[:, 3], 'gt_xywh': gb[b, :g], 'gt_area': ga[b, :g], 'gt_iscrowd': gi[b, :g],
                       'gt_cat': gk[b, :g], 'iou': cnp.bb_iou(xywh, gb[b, :g], gi[b, :g])})
    params = dict(cnp.default_params(), max_dets=[1, 100, 1000])
    want = knp.evaluate(images, 2, params, use_cats=False)
    n = cnp.stat_counts(want['precision'], want['recall'], want['specs'])
    print("proposal stats", stats, "host", want['stats'])
    assert np.all(np.abs(stats - want['stats']) <= 2.0 * n * 2.0 ** -53) and stats[8] > 0, (stats, want['stats'])
    with pytest.raises(ValueError):
        evaluate.coco_stats([item], pred, new(), proposals=True)               # a use_cats=True evaluator
    with pytest.raises(ValueError):
        evaluate.coco_stats([item], pred, CocoEvaluator(1, 'keypoints', num_keypoints=17, max_images=2, max_dets_per_image=P, max_gts_per_image=G, device=cuda))


# -------------------------------------------------------------------------------------------------------------------- merging
def test_merged_halves_equal_one_evaluator(cuda):
    from scda_amd.coco_eval import CocoEvaluator
    # keypoints
    images = evaluated('kp_random')[0]
    n = len(images)
    whole = _default_kp_run('kp_random', cuda)
    halves = []
    for idx in (list(range(0, n, 2)), list(range(1, n, 2))):
        ev = _kp_evaluator('kp_random', cuda, max_images=n, debug=False)
        args, kw = _kp_batch(images, idx, ev.D, ev.G, cuda)
        ev.add(*args, **kw)
        halves.append(ev)
    merged = _kp_evaluator('kp_random', cuda, max_images=n, debug=False).absorb(halves)
    got = {k: v.cpu().numpy() for k, v in merged.accumulate().items()}
    for k in ('precision', 'recall', 'scores'):
        assert got[k].tobytes() == whole[k].tobytes(), k
    assert merged.summarize().tobytes() == whole['stats'].tobytes() and np.array_equal(merged.npig.cpu().numpy(), whole['npig'])
    other = _kp_evaluator('kp_random', cuda, max_images=n, debug=False, params={'sigmas': knp.default_params()['sigmas'] * 2})
    with pytest.raises(ValueError):
        other.absorb(halves)                                                  # other sigmas
    # useCats = 0
    whole, _ = _nocat_run('nocat_props', cuda, xyxy_as_xywh=True)
    halves = [_nocat_run('nocat_props', cuda, order=idx, xyxy_as_xywh=True, max_images=4)[1] for idx in ([0, 2], [1, 3])]
    D, G = NOCAT_CAPS['nocat_props']
    new = lambda **kw: CocoEvaluator(1, 'bbox', max_images=4, max_dets_per_image=D, max_gts_per_image=G, device=cuda,     # noqa: E731
                                     params={'max_dets': [1, 100, 1000]}, **kw)
    merged = new(use_cats=False).absorb(halves)
    got = {k: v.cpu().numpy() for k, v in merged.accumulate().items()}
    for k in ('precision', 'recall', 'scores'):
        assert got[k].tobytes() == whole[k].tobytes(), k
    assert merged.summarize().tobytes() == whole['stats'].tobytes()
    with pytest.raises(ValueError):
        new().absorb(halves)                                                  # use_cats differs


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(cuda):
    from scda_amd.coco_eval import CocoEvaluator
    images = evaluated('kp_rules')[0]
    with pytest.raises(ValueError):
        CocoEvaluator(1, 'keypoints', device=cuda)                            # Kp has no default
    with pytest.raises(ValueError):
        CocoEvaluator(1, 'keypoints', num_keypoints=16, device=cuda)          # 17 sigmas
    with pytest.raises(ValueError):
        CocoEvaluator(4, 'bbox', num_keypoints=17, device=cuda)
    with pytest.raises(ValueError):
        CocoEvaluator(1, 'keypoints', num_keypoints=17, device=cuda, use_cats=False)
    with pytest.raises(ValueError):
        CocoEvaluator(4, 'bbox', device=cuda, params={'area_rng': knp.default_params()['area_rng']})         # A = 3 for 'bbox'
    with pytest.raises(ValueError):
        CocoEvaluator(1, 'keypoints', num_keypoints=33, device=cuda, params={'sigmas': np.ones(33)})
    ev = _kp_evaluator('kp_rules', cuda, debug=False)
    args, kw = _kp_batch(images, [0, 1], ev.D, ev.G, cuda)
    with pytest.raises(ValueError):
        ev.add(*args)                                                         # no keypoints
    with pytest.raises(ValueError):
        ev.add(*args, **dict(kw, gt_num_keypoints=None))
    with pytest.raises(ValueError):
        ev.add(*args, **dict(kw, keypoints=kw['keypoints'][:, :, :16].contiguous()))          # another Kp
    with pytest.raises(ValueError):
        ev.add_proposals(args[0], torch.zeros(2, ev.D, 6, device=cuda), *args[2:])            # not a use_cats=False 'bbox' evaluator
    assert ev.n_images == 0 and int(ev.seen.sum()) == 0 and int(ev.npig.sum()) == 0
    ok = CocoEvaluator(1, 'keypoints', num_keypoints=17, max_images=2, max_dets_per_image=ev.D, max_gts_per_image=ev.G, device=cuda,
                       params={'area_rng': knp.default_params()['area_rng']})
    assert ok.A == 3 and ok.stats.numel() == 10


# -------------------------------------------------------------------------------------------------------- unchanged behaviour
def test_the_new_match_entry_with_a_null_ignore_equals_the_old_one(cuda):
    """random_bbox of the existing fixture through scda_coco_match_hip and through scda_coco_match_ign_hip with a null ignore pointer:
    identical rank, bits, npig, seen and debug rows, hence identical precision / recall / scores"""
    from scda_amd import native as N
    from scda_amd.coco_eval import CocoEvaluator
    from test_coco_eval_gpu import CAPS, _batch
    z = segm_fixture()
    images, K, params = cnp.load_set(z, 'random_bbox')
    D, G = CAPS['random_bbox']
    args, _ = _batch(images, list(range(len(images))), D, G, cuda)
    ev = CocoEvaluator(K, 'bbox', max_images=len(images), max_dets_per_image=D, max_gts_per_image=G, device=cuda,
                       params={'area_rng': params['area_rng']}, debug=True)
    ev.add(*args)
    acc = {k: v.cpu().numpy().copy() for k, v in ev.accumulate().items()}
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(acc[key], z['random_bbox_' + key]), key
    ids, det, dc, gb, ga, gi, gk, gc = args
    outs = []
    for entry in (N.coco_match, N.coco_match_ign):
        rank, bits = torch.zeros_like(ev.rank), torch.zeros_like(ev.bits)
        npig, seen, dbg = torch.zeros_like(ev.npig), torch.zeros_like(ev.seen), torch.full_like(ev.debug_match, -1)
        extra = (None,) if entry is N.coco_match_ign else ()
        entry(ev._iou, dc, ev.cat, ev.score, ev.area, gc, gk, ga, gi, *extra, K, ev.d_iou_thrs, ev.d_area_rng, 100, rank, bits, npig, seen,
              dbg_match=dbg)
        outs.append([t.cpu().numpy() for t in (rank, bits, npig, seen, dbg)])
    for a, b, c in zip(outs[0], outs[1], (ev.rank, ev.bits, ev.npig, ev.seen, ev.debug_match)):
        assert a.tobytes() == b.tobytes() == c.cpu().numpy().tobytes()
