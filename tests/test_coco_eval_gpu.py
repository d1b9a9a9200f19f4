"""COCO AP on the MI355X (scda_amd/csrc/coco_eval.hip, scda_amd/coco_eval.py) against the arrays recorded from the reference's own
cocoeval.py / maskApi.c (tests/golden/coco_eval_ref.npz): box IoU, matching and accumulation bit for bit, the stats within the bound
between two summation orders, independence of the order and batching of the images, 'segm' through native.mask_iou on packed planes,
the capacity contract, the path whose IoU block does not fit LDS, and Predictor(masks=True, rle=True) -> CocoEvaluator end to end
against the numpy statement (tests/coco_eval_np.py)."""
import numpy as np
import pytest
import torch

import coco_eval_np as cnp
from test_coco_eval_rules import SETS, evaluated, fixture

pytestmark = pytest.mark.gpu

CAPS = {'rules': (128, 16), 'random_bbox': (100, 12), 'random_segm': (32, 8)}     # (detection slots, GT slots) per image


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _batch(images, idx, D, G, cuda, z=None, name=None):
    """the images idx as the tensors CocoEvaluator.add takes (padding rows zero)"""
    B = len(idx)
    det = np.zeros((B, D, 7), np.float32); dc = np.zeros(B, np.int32); gc = np.zeros(B, np.int32)
    gb = np.zeros((B, G, 4), np.float64); ga = np.zeros((B, G), np.float64); gi = np.zeros((B, G), np.uint8); gk = np.zeros((B, G), np.int32)
    for b, i in enumerate(idx):
        im = images[i]
        d, g = len(im['dt_score']), len(im['gt_cat'])
        dc[b], gc[b] = d, g
        det[b, :, 0] = b
        det[b, :d, 1:5], det[b, :d, 5], det[b, :d, 6] = im['dt_corners'], im['dt_score'], im['dt_cat']
        gb[b, :g], ga[b, :g], gi[b, :g], gk[b, :g] = im['gt_xywh'], im['gt_area'], im['gt_iscrowd'], im['gt_cat']
    args = [_dev(np.asarray([images[i]['image_id'] for i in idx], np.int32), cuda)] + [_dev(a, cuda) for a in (det, dc, gb, ga, gi, gk, gc)]
    kw = {}
    if z is not None and name + '_dt_bits' in z:
        H, Wd = z[name + '_dt_bits'].shape[1:]
        mb = np.zeros((B, D, H, Wd), np.uint32); gm = np.zeros((B, G, H, Wd), np.uint32); da = np.zeros((B, D), np.int32)
        for b, i in enumerate(idx):
            im = images[i]
            mb[b, :dc[b]], gm[b, :gc[b]] = z[name + '_dt_bits'][im['dt']], z[name + '_gt_bits'][im['gt']]
            da[b, :dc[b]] = im['dt_area'].astype(np.int32)
        kw = {'mask_bits': _dev(mb.view(np.int32), cuda), 'gt_mask_bits': _dev(gm.view(np.int32), cuda), 'det_areas': _dev(da, cuda),
              'sizes': tuple(int(v) for v in z[name + '_size'])}
    return args, kw


def _run(name, cuda, order=None, batch=None, debug=True):
    """the set through a CocoEvaluator -> host arrays, the per-detection ones back in the fixture's image order"""
    from scda_amd.coco_eval import CocoEvaluator
    z = fixture()
    images, K, params = cnp.load_set(z, name)
    D, G = CAPS[name]
    order = list(range(len(images))) if order is None else list(order)
    batch = len(images) if batch is None else batch
    ev = CocoEvaluator(K, 'segm' if name == 'random_segm' else 'bbox', max_images=len(images), max_dets_per_image=D, max_gts_per_image=G,
                       device=cuda, params={'area_rng': params['area_rng']}, debug=debug)
    for s in range(0, len(order), batch):
        args, kw = _batch(images, order[s:s + batch], D, G, cuda, z, name)
        ev.add(*args, **kw)
    res = {k: v.cpu().numpy().copy() for k, v in ev.accumulate().items()}
    res['stats'] = ev.summarize()
    res['npig'] = ev.npig.cpu().numpy()
    slot = {i: s for s, i in enumerate(order)}
    pick = lambda t: np.concatenate([t[slot[i], :len(images[i]['dt_score'])] for i in range(len(images))])   # noqa: E731
    res['rank'], res['bits'] = pick(ev.rank.cpu().numpy()), pick(ev.bits.cpu().numpy().view(np.uint32))
    if debug:
        res['match'] = pick(ev.debug_match.cpu().numpy())
    return res


_RUNS = {}


def _default_run(name, cuda):
    if name not in _RUNS:
        _RUNS[name] = _run(name, cuda)
    return _RUNS[name]


@pytest.mark.parametrize("name", ('rules', 'random_bbox'))
def test_box_iou_is_bit_equal_to_the_reference(cuda, name):
    from scda_amd import native as N
    images = cnp.load_set(fixture(), name)[0]
    D, G = CAPS[name]
    args, _ = _batch(images, list(range(len(images))), D, G, cuda)
    xywh = np.zeros((len(images), D, 4))
    for b, im in enumerate(images):
        xywh[b, :len(im['dt_score'])] = im['dt_xywh']
    got = N.coco_box_iou(_dev(xywh, cuda), args[2], args[3], args[7], args[5]).cpu().numpy()
    for b, im in enumerate(images):
        g, d = im['iou'].shape if im['iou'].size else (0, 0)
        assert np.array_equal(got[b, :g, :d], im['iou'].reshape(g, d)), (name, b)


@pytest.mark.parametrize("name", SETS)
def test_matching_equals_the_recorded_eval_imgs(cuda, name):
    z = fixture()
    got = _default_run(name, cuda)
    T = 10
    part = z[name + '_rank'] >= 0
    assert np.array_equal(got['rank'][part], z[name + '_rank'][part]) and (got['rank'][~part] >= 100).all()
    assert np.array_equal(got['match'], z[name + '_match'])
    t = np.arange(T)
    matched = (got['bits'][:, :, None] >> t) & 1
    ignored = (got['bits'][:, :, None] >> (16 + t)) & 1
    assert np.array_equal(matched, (z[name + '_match'] >= 0).astype(np.uint32))
    assert np.array_equal(ignored, z[name + '_ignore'].astype(np.uint32))
    assert np.array_equal(got['npig'], z[name + '_npig'])


@pytest.mark.parametrize("name", SETS)
def test_accumulate_is_bit_equal_and_stats_within_the_bound(cuda, name):
    z = fixture()
    got = _default_run(name, cuda)
    for key in ('precision', 'recall', 'scores'):
        assert got[key].dtype == np.float64 and got[key].shape == z[name + '_' + key].shape
        assert np.array_equal(got[key], z[name + '_' + key]), (key, int((got[key] != z[name + '_' + key]).sum()))
    res = evaluated(name)[3]
    n = cnp.stat_counts(z[name + '_precision'], z[name + '_recall'], res['specs'])
    print(name, "stats", got['stats'], "max |diff|", np.abs(got['stats'] - z[name + '_stats']).max())
    assert np.all(np.abs(got['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53), (got['stats'], z[name + '_stats'])


@pytest.mark.parametrize("name", ('rules', 'random_bbox'))
def test_order_and_batching_of_the_images_do_not_matter(cuda, name):
    z = fixture()
    n = len(z[name + '_image_ids'])
    base = _default_run(name, cuda)
    perm = np.random.RandomState(5).permutation(n)
    runs = [_run(name, cuda, debug=False), _run(name, cuda, order=perm, batch=3, debug=False), _run(name, cuda, order=perm[::-1], batch=1, debug=False)]
    for r in runs:
        for key in ('precision', 'recall', 'scores', 'stats', 'npig', 'rank', 'bits'):
            assert r[key].tobytes() == base[key].tobytes(), key


def test_converted_inputs_give_the_bytes_of_device_inputs(cuda):
    """add() takes device tensors of the stated types as they are and converts anything else (eval_base.StreamingEvaluator._dev, through
    native.upload): host numpy arrays, device tensors of another dtype (each wide enough to hold the values exactly) and non-contiguous
    ones give the arrays of the all-device run byte for byte"""
    from scda_amd.coco_eval import CocoEvaluator
    images, K, params = cnp.load_set(fixture(), 'rules')
    D, G = CAPS['rules']
    base = _default_run('rules', cuda)
    args, _ = _batch(images, list(range(len(images))), D, G, cuda)
    ids, det, dc, gb, ga, gi, gk, gc = args
    wide = lambda t: torch.stack([t, t], -1)[..., 0]        # noqa: E731  (a non-contiguous view with the same values)
    assert not wide(gb).is_contiguous()
    variants = {'host numpy': [a.cpu().numpy() for a in args],
                'other dtypes': [ids.long(), det.double(), dc.long(), wide(gb), wide(ga), gi.int(), gk.long(), gc.long()]}
    for what, given in variants.items():
        ev = CocoEvaluator(K, 'bbox', max_images=len(images), max_dets_per_image=D, max_gts_per_image=G, device=cuda,
                           params={'area_rng': params['area_rng']})
        ev.add(*given)
        got = ev.accumulate()
        for key in ('precision', 'recall', 'scores'):
            assert got[key].cpu().numpy().tobytes() == base[key].tobytes(), (what, key)


def test_segm_ious_come_from_mask_iou_on_packed_planes(cuda):
    from scda_amd import native as N
    z = fixture()
    images = cnp.load_set(z, 'random_segm')[0]
    size = tuple(int(v) for v in z['random_segm_size'])
    for im in images[:4]:
        dt = _dev(z['random_segm_dt_bits'][im['dt']].view(np.int32), cuda)
        gt = _dev(z['random_segm_gt_bits'][im['gt']].view(np.int32), cuda)
        iou, _ = N.mask_iou(dt, gt, size, iscrowd=_dev(im['gt_iscrowd'], cuda))
        assert np.array_equal(iou.cpu().numpy(), im['iou'])


def test_capacity_violations_raise_before_anything_runs(cuda):
    from scda_amd.coco_eval import CocoEvaluator
    images = cnp.load_set(fixture(), 'rules')[0]
    with pytest.raises(ValueError):
        CocoEvaluator(4, 'keypoints', device=cuda)
    with pytest.raises(ValueError):
        CocoEvaluator(300, 'bbox', device=cuda)
    with pytest.raises(ValueError):
        CocoEvaluator(4, 'bbox', max_dets_per_image=2048, device=cuda)
    ev = CocoEvaluator(4, 'bbox', max_images=2, max_dets_per_image=128, max_gts_per_image=16, device=cuda)
    args, _ = _batch(images, [0, 1, 2], 128, 16, cuda)
    with pytest.raises(ValueError):
        ev.add(*args)                                                         # three images into two slots
    args, _ = _batch(images, [0], 64, 16, cuda)
    with pytest.raises(ValueError):
        ev.add(*args)                                                         # another top_n
    args, _ = _batch(images, [0], 128, 8, cuda)
    with pytest.raises(ValueError):
        ev.add(*args)                                                         # another Gcap
    with pytest.raises(ValueError):
        CocoEvaluator(4, 'segm', max_images=2, max_dets_per_image=128, max_gts_per_image=16, device=cuda).add(*_batch(images, [0], 128, 16, cuda)[0])
    assert ev.n_images == 0 and int(ev.seen.sum()) == 0
    with pytest.raises(ValueError):
        ev.accumulate()


def _crowded_image(rs, image_id, n_det, n_gt, K):
    """many detections and GTs of few categories in one image: the (image, category) IoU block exceeds the LDS stage"""
    gx, gy = rs.uniform(0, 400, n_gt), rs.uniform(0, 200, n_gt)
    gw, gh = rs.uniform(10, 120, n_gt), rs.uniform(10, 120, n_gt)
    gt_xywh = np.round(np.stack([gx, gy, gw, gh], 1), 1)
    pick = rs.randint(0, n_gt, n_det)
    j = rs.normal(0, 0.15, (n_det, 4))
    x1 = gt_xywh[pick, 0] + j[:, 0] * gt_xywh[pick, 2]; y1 = gt_xywh[pick, 1] + j[:, 1] * gt_xywh[pick, 3]
    corners = np.stack([x1, y1, x1 + gt_xywh[pick, 2] * np.exp(j[:, 2]), y1 + gt_xywh[pick, 3] * np.exp(j[:, 3])], 1).astype(np.float32)
    xywh = cnp.xywh_from_corners(corners)
    crowd = (rs.rand(n_gt) < 0.2).astype(np.uint8)
    im = {'image_id': image_id, 'dt_corners': corners, 'dt_xywh': xywh, 'dt_score': np.round(rs.uniform(0.05, 1, n_det), 2).astype(np.float32),
          'dt_cat': rs.randint(1, K + 1, n_det).astype(np.int32), 'dt_area': xywh[:, 2] * xywh[:, 3], 'gt_xywh': gt_xywh,
          'gt_area': gt_xywh[:, 2] * gt_xywh[:, 3] * rs.choice([0.6, 1.0], n_gt), 'gt_iscrowd': crowd, 'gt_cat': rs.randint(1, K + 1, n_gt).astype(np.int32)}
    im['iou'] = cnp.bb_iou(xywh, gt_xywh, crowd)
    return im


def test_blocks_beyond_the_lds_stage_equal_the_statement(cuda):
    from scda_amd.coco_eval import CocoEvaluator
    rs = np.random.RandomState(11)
    K, D, G = 2, 192, 96
    images = [_crowded_image(rs, 7, 180, 90, K), _crowded_image(rs, 3, 40, 5, K)]
    assert min((images[0]['dt_cat'] == 1).sum(), 100) * (images[0]['gt_cat'] == 1).sum() > 2048              # kIouLds of coco_eval.hip
    want = cnp.evaluate(images, K)
    ev = CocoEvaluator(K, 'bbox', max_images=2, max_dets_per_image=D, max_gts_per_image=G, device=cuda, debug=True)
    args, _ = _batch(images, [0, 1], D, G, cuda)
    ev.add(*args)
    got = {k: v.cpu().numpy() for k, v in ev.accumulate().items()}
    for b, (im, e) in enumerate(zip(images, want['per_image'])):
        n = len(im['dt_score'])
        assert np.array_equal(ev.rank[b, :n].cpu().numpy(), e['rank'])
        assert np.array_equal(ev.debug_match[b, :n].cpu().numpy(), e['match'])
    for key in ('precision', 'recall', 'scores'):
        assert np.array_equal(got[key], want[key]), key
    n = cnp.stat_counts(want['precision'], want['recall'], want['specs'])
    assert np.all(np.abs(ev.summarize() - want['stats']) <= 2.0 * n * 2.0 ** -53)


def test_predictor_into_evaluator_end_to_end(cuda):
    """a seeded mask-branch detector through Predictor(masks=True, rle=True) into both evaluators, synthetic ground truth cut from its own
    detections, against the numpy statement on the same rows"""
    from scda_amd import infer, native as N
    from scda_amd.coco_eval import CocoEvaluator
    from test_mask_infer_gpu import H_IMG, W_IMG, _images, _mask_detector
    det, cfg = _mask_detector(cuda)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.0], [H_IMG, W_IMG, 1.0]])
    out = infer.Predictor(det, cfg, masks=True, rle=True)(x, info)
    dets, counts = out[2].cpu().numpy(), out[3].cpu().numpy()
    top_n, K, G = dets.shape[1], int(cfg['shared']['num_classes']) - 1, 8
    assert counts.min() > 0
    words = out[4].cpu().numpy().view(np.uint32)
    area = out[5]['area'].cpu().numpy()
    # ground truth: every third detection (its box grown by a pixel, its own mask), the second one a crowd
    gb = np.zeros((2, G, 4)); ga = np.zeros((2, G)); gi = np.zeros((2, G), np.uint8); gk = np.zeros((2, G), np.int32); gc = np.zeros(2, np.int32)
    gm = np.zeros((2, G) + words.shape[2:], np.uint32)
    for b in range(2):
        src = list(range(0, int(counts[b]), 3))[:G]
        gc[b] = len(src)
        for g, j in enumerate(src):
            x1, y1, x2, y2 = dets[b, j, 1:5].astype(np.float64)
            gb[b, g] = (x1 - 1, y1, x2 - x1 + 1, y2 - y1 + 1)
            ga[b, g], gi[b, g], gk[b, g], gm[b, g] = gb[b, g, 2] * gb[b, g, 3], g == 1, int(dets[b, j, 6]), words[b, j]
    ids = torch.tensor([12, 5], dtype=torch.int32, device=cuda)
    gts = [_dev(a, cuda) for a in (gb, ga, gi, gk, gc)]
    for iou_type in ('bbox', 'segm'):
        ev = CocoEvaluator(K, iou_type, max_images=2, max_dets_per_image=top_n, max_gts_per_image=G, device=cuda)
        kw = {} if iou_type == 'bbox' else {'mask_bits': out[4], 'det_areas': out[5]['area'], 'gt_mask_bits': _dev(gm.view(np.int32), cuda),
                                            'sizes': (H_IMG, W_IMG)}
        ev.add(ids, out[2], out[3], *gts, **kw)
        got = {k: v.cpu().numpy() for k, v in ev.accumulate().items()}
        stats = ev.summarize()
        images = []
        for b in range(2):
            n, g = int(counts[b]), int(gc[b])
            xywh = cnp.xywh_from_corners(dets[b, :n, 1:5])
            if iou_type == 'bbox':
                iou, dt_area = cnp.bb_iou(xywh, gb[b, :g], gi[b, :g]), xywh[:, 2] * xywh[:, 3]
            else:
                iou = N.mask_iou(out[4][b, :n].contiguous(), _dev(gm[b, :g].view(np.int32), cuda), (H_IMG, W_IMG),
                                 iscrowd=_dev(gi[b, :g], cuda))[0].cpu().numpy()
                dt_area = area[b, :n].astype(np.float64)
            images.append({'image_id': int(ids[b]), 'dt_xywh': xywh, 'dt_score': dets[b, :n, 5], 'dt_cat': dets[b, :n, 6].astype(np.int32),
                           'dt_area': dt_area, 'gt_xywh': gb[b, :g], 'gt_area': ga[b, :g], 'gt_iscrowd': gi[b, :g], 'gt_cat': gk[b, :g], 'iou': iou})
        want = cnp.evaluate(images, K)
        for key in ('precision', 'recall', 'scores'):
            assert np.array_equal(got[key], want[key]), (iou_type, key)
        n = cnp.stat_counts(want['precision'], want['recall'], want['specs'])
        assert np.all(np.abs(stats - want['stats']) <= 2.0 * n * 2.0 ** -53) and stats[0] > 0, (iou_type, stats)
