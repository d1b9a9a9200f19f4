"""tests/coco_kps_np.py (the numpy restatement of the keypoint / OKS and useCats = 0 rules in include/scda_ops.h) against the arrays
recorded from the reference's own cocoeval.py in tests/golden/coco_kps_ref.npz, and the host-side pieces of the feature: the ten
keypoint specs, the 12 specs over maxDets [1, 100, 1000], flatten_annotations(keypoints=True).  No GPU."""
import os

import numpy as np
import pytest

import coco_eval_np as cnp
import coco_kps_np as knp
from conftest import ROOT

KP_SETS = ('kp_rules', 'kp_random', 'kp_blocks')
NOCAT_SETS = ('nocat_rules', 'nocat_props', 'nocat_xyxy', 'nocat_segm')
XYXY_SETS = ('nocat_props', 'nocat_xyxy')          # recorded as the reference's 'proposal' run: [x1, y1, x2, y2] handed over as xywh
OKS_TOL = 1e-13     # at most 17 terms in [0, 1], each exp within 1 ulp (2.2e-16) on either side, the reordered sum within 17 * 2^-53
#                     relative: below 1e-14 together; the bound is ten times that
_CACHE = {}


def fixture():
    if 'z' not in _CACHE:
        _CACHE['z'] = dict(np.load(os.path.join(ROOT, "tests", "golden", "coco_kps_ref.npz")))
    return _CACHE['z']


def segm_fixture():
    if 'zs' not in _CACHE:
        _CACHE['zs'] = dict(np.load(os.path.join(ROOT, "tests", "golden", "coco_eval_ref.npz")))
    return _CACHE['zs']


def nocat_inputs(name):
    """(images, K, params, recorded-array prefix source) of a useCats = 0 set; nocat_segm's inputs are random_segm's"""
    if name == 'nocat_segm':
        return cnp.load_set(segm_fixture(), 'random_segm')
    return knp.load_box_set(fixture(), name, xyxy_as_xywh=name in XYXY_SETS)


def evaluated(name):
    """(images, K, params, coco_kps_np's result), computed once per set and not modified"""
    if name not in _CACHE:
        if name in KP_SETS:
            images, K, params = knp.load_kp_set(fixture(), name)
            res = knp.evaluate(images, K, params, keypoints=True)
        else:
            images, K, params = nocat_inputs(name)
            res = knp.evaluate(images, K, params, use_cats=False)
        _CACHE[name] = (images, K, params, res)
    return _CACHE[name]


def given_order(name, res, images):
    """the per-image arrays of a useCats = 0 result back in the order GIVEN, as the golden file records them: rank (-1: no part),
    match as given GT rows, ignore"""
    z = fixture()
    A, T = z[name + '_match'].shape[1:]
    rank, match, ignore = [], [], []
    for im, e, (pd, pg) in zip(images, res['per_image'], res['perms']):
        n = len(im['dt_score'])
        r, m, i = np.full(n, -1, np.int32), np.full((n, A, T), -1, np.int32), np.zeros((n, A, T), np.uint8)
        r[pd] = e['rank']
        m[pd] = np.where(e['match'] >= 0, pg[np.maximum(e['match'], 0)] if len(pg) else -1, -1)
        i[pd] = e['ignore']
        rank.append(r); match.append(m); ignore.append(i)
    return np.concatenate(rank), np.concatenate(match), np.concatenate(ignore)


def test_keypoint_parameters_are_the_references():
    p = knp.default_params()
    assert p['max_dets'] == [20] and p['area_rng'].tolist() == [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
    assert len(p['sigmas']) == 17 and p['sigmas'][0] == .26 / 10.0 and p['sigmas'][11] == 1.07 / 10.0
    assert np.array_equal(fixture()['kp_rules_area_rng'], p['area_rng'])


def test_kps_stat_specs():
    """the product's ten specs (scda_amd.coco_eval.kps_stat_specs) and the restatement's, each against _summarizeKps written out"""
    from scda_amd import coco_eval as ce
    p = knp.default_params()
    for mod in (ce, knp):
        s = mod.kps_stat_specs(p['iou_thrs'], [20])
        assert s.shape == (10, 4) and s[:, 0].tolist() == [1] * 5 + [0] * 5 and s[:, 3].tolist() == [0] * 10
        assert s[:5, 1].tolist() == [-1, 0, 5, -1, -1] and s[5:, 1].tolist() == [-1, 0, 5, -1, -1]
        assert s[:5, 2].tolist() == [0, 0, 0, 1, 2] and s[5:, 2].tolist() == [0, 0, 0, 1, 2]
        assert mod.kps_stat_specs(p['iou_thrs'], [5, 20, 50])[:, 3].tolist() == [1] * 10
        assert mod.kps_stat_specs(p['iou_thrs'], [10, 100])[:, 1].tolist() == [-2] * 10          # no 20: every stat is -1
        assert mod.kps_stat_specs(np.array([.6, .7]), [20])[:3, 1].tolist() == [-1, -2, -2]


def test_stat_specs_over_the_proposal_max_dets():
    """the 12 specs over maxDets [1, 100, 1000], as a use_cats=False evaluator's parameters give them (default_params keeps its
    detection values when called with an iou_type, the argument the feature adds)"""
    from scda_amd import coco_eval as ce
    p = ce.default_params('bbox')
    assert p['max_dets'] == [1, 10, 100] and np.array_equal(p['iou_thrs'], cnp.default_params()['iou_thrs'])
    for mod in (ce, cnp):
        s = mod.stat_specs(p['iou_thrs'], [1, 100, 1000])
        assert s[0].tolist() == [1, -1, 0, 1]                                # stat 0: the entry EQUAL to 100
        assert s[1:6, 3].tolist() == [2] * 5 and s[6:9, 3].tolist() == [0, 1, 2] and s[9:, 3].tolist() == [2] * 3


def test_product_specs_and_parameters_equal_the_restatement():
    from scda_amd import coco_eval as ce
    p, q = ce.default_params('keypoints'), knp.default_params()
    assert sorted(p) == sorted(q) and all(np.array_equal(np.asarray(p[k]), np.asarray(q[k])) for k in p)
    assert sorted(ce.default_params()) == sorted(cnp.default_params()) and 'sigmas' not in ce.default_params()
    for md in ([20], [5, 20, 50], [10, 100]):
        assert np.array_equal(ce.kps_stat_specs(p['iou_thrs'], md), knp.kps_stat_specs(p['iou_thrs'], md))
    assert np.array_equal(ce.stat_specs(p['iou_thrs'], [1, 100, 1000]), cnp.stat_specs(p['iou_thrs'], [1, 100, 1000]))


@pytest.mark.parametrize("name", KP_SETS)
def test_oks_equals_the_references(name):
    images = evaluated(name)[0]
    worst = 0.0
    for im in images:
        got, want = im['iou'], im['oks_ref']
        exact = (want == 1.0) | (want == 0.0)
        assert np.array_equal(got[exact], want[exact])
        if got.size:
            worst = max(worst, float(np.abs(got - want).max()))
    print(name, "max |oks - reference|", worst)
    assert worst <= OKS_TOL
    if name == 'kp_rules':
        o = np.concatenate([im['oks_ref'].reshape(-1) for im in images])
        assert (o == 1.0).sum() >= 2 and (o == 0.0).any()


@pytest.mark.parametrize("name", KP_SETS)
def test_keypoint_rows_and_ignore_flags(name):
    z = fixture()
    images = evaluated(name)[0]
    for im in images:
        k = im['dt_kps'].astype(np.float64)
        for d in range(len(k)):                                              # loadRes, literally
            x0, x1, y0, y1 = np.min(k[d, :, 0]), np.max(k[d, :, 0]), np.min(k[d, :, 1]), np.max(k[d, :, 1])
            assert im['dt_xywh'][d].tolist() == [x0, y0, x1 - x0, y1 - y0] and im['dt_area'][d] == (x1 - x0) * (y1 - y0)
    flags = np.concatenate([im['gt_ignore'] for im in images])
    # area range 0 is [0, 1e10]: gtIgnore there is the flag itself
    assert np.array_equal(flags, z[name + '_gt_ignore'][:, 0])


@pytest.mark.parametrize("name", KP_SETS)
def test_keypoint_matching_equals_the_recorded_eval_imgs(name):
    z = fixture()
    images, K, params, res = evaluated(name)
    rank = np.concatenate([e['rank'] for e in res['per_image']])
    part = z[name + '_rank'] >= 0
    assert np.array_equal(rank[part], z[name + '_rank'][part]) and (rank[~part] >= params['max_dets'][-1]).all()
    assert np.array_equal(np.concatenate([e['match'] for e in res['per_image']]), z[name + '_match'])
    assert np.array_equal(np.concatenate([e['ignore'] for e in res['per_image']]).astype(np.uint8), z[name + '_ignore'])
    assert np.array_equal(np.concatenate([e['gt_ignore'] for e in res['per_image']]).astype(np.uint8), z[name + '_gt_ignore'])
    assert np.array_equal(sum(e['npig'] for e in res['per_image']), z[name + '_npig'])


@pytest.mark.parametrize("name", NOCAT_SETS)
def test_regroup_order_and_matching_equal_the_recorded_eval_imgs(name):
    z = fixture()
    images, K, params, res = evaluated(name)
    assert np.array_equal(np.concatenate([p[0] for p in res['perms']]), z[name + '_dt_order'])
    assert np.array_equal(np.concatenate([p[1] for p in res['perms']]), z[name + '_gt_order'])
    assert [len(p[0]) for p in res['perms']] == z[name + '_dt_live'].tolist()
    rank, match, ignore = given_order(name, res, images)
    part = z[name + '_rank'] >= 0
    assert np.array_equal(rank[part], z[name + '_rank'][part])
    assert ((rank[~part] >= params['max_dets'][-1]) | (rank[~part] == -1)).all()
    assert np.array_equal(match, z[name + '_match']) and np.array_equal(ignore, z[name + '_ignore'])
    assert np.array_equal(sum(e['npig'] for e in res['per_image']), z[name + '_npig'])


@pytest.mark.parametrize("name", KP_SETS + NOCAT_SETS)
def test_accumulate_equals_the_recorded_eval_and_stats_within_the_bound(name):
    z = fixture()
    res = evaluated(name)[3]
    for key in ('precision', 'recall', 'scores'):
        assert res[key].dtype == np.float64 and np.array_equal(res[key], z[name + '_' + key]), key
    n = cnp.stat_counts(res['precision'], res['recall'], res['specs'])
    assert len(res['stats']) == (10 if name in KP_SETS else 12)
    assert np.all(np.abs(res['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53), (res['stats'], z[name + '_stats'])
    assert ((z[name + '_stats'] == -1) == (n == 0)).all()


def test_the_golden_sets_cover_their_edges():
    z = fixture()
    assert z['kp_blocks_dt_counts'].tolist()[:4] == [1, 255, 256, 257] and z['kp_blocks_gt_counts'].max() == 12
    assert (z['kp_rules_rank'] == -1).sum() == 5 and z['kp_rules_dt_counts'].max() == 25
    k1 = (z['kp_random_gt_kps'][:, :, 2] > 0).sum(1)
    assert (k1 == 0).any() and (z['kp_random_gt_iscrowd'] == 1).any()
    assert (z['kp_rules_gt_num_kps'] == 0).any() and ((z['kp_rules_gt_num_kps'] > 0) & ((z['kp_rules_gt_kps'][:, :, 2] > 0).sum(1) == 0)).any()
    assert z['nocat_props_max_dets'].tolist() == [1, 100, 1000] and z['nocat_props_dt_counts'].tolist()[:3] == [1010, 300, 0]
    assert z['nocat_props_gt_counts'][1] * 300 > 2048                       # kIouLds of coco_eval.hip
    assert z['nocat_rules_dt_order'][:3].tolist() == [2, 1, 0]
    # nocat_xyxy: (x2, y2) read as (w, h) loses the first proposal's match and gives the second one (whose x2 < x1: it is a box only
    # under that reading); with true widths the restatement has it the other way round
    assert z['nocat_xyxy_match'][:, 0, 0].tolist() == [-1, 1, 0]
    images, K, params = knp.load_box_set(z, 'nocat_xyxy', xyxy_as_xywh=False)
    true_w = knp.evaluate(images, K, params, use_cats=False)
    assert true_w['per_image'][0]['match'][:, 0, 0].tolist() == [0, -1]
    assert tuple(z['nocat_props_precision'].shape) == (10, 101, 1, 4, 3)


def _ann(kps=None, num=None):
    a = {'segmentation': [[0, 0, 10, 0, 10, 10]], 'bbox': [0, 0, 10, 10], 'area': 50.0, 'iscrowd': 0, 'category_id': 1}
    if kps is not None:
        a['keypoints'] = kps
    if num is not None:
        a['num_keypoints'] = num
    return a


def test_flatten_annotations_with_keypoints():
    from scda_amd import coco_gt
    kps = [float(v) for v in range(51)]
    anns = [[_ann(kps, 4), _ann(kps[::-1], 0)], [], [_ann(kps, 17)]]
    old = coco_gt.flatten_annotations(anns, (20, 20), 3)
    assert sorted(old) == ['gt_areas', 'gt_boxes', 'gt_categories', 'gt_counts', 'gt_iscrowd', 'poly_first', 'poly_plane', 'rle_counts',
                           'rle_first', 'rle_plane', 'sizes', 'xy']
    flat = coco_gt.flatten_annotations(anns, (20, 20), 3, keypoints=True)
    assert sorted(set(flat) - set(old)) == ['gt_keypoints', 'gt_num_keypoints'] and all(np.array_equal(flat[k], old[k]) for k in old)
    assert flat['gt_keypoints'].shape == (3, 3, 17, 3) and flat['gt_keypoints'].dtype == np.float64
    assert flat['gt_num_keypoints'].shape == (3, 3) and flat['gt_num_keypoints'].dtype == np.int32
    assert flat['gt_keypoints'][0, 0].reshape(-1).tolist() == kps and flat['gt_keypoints'][0, 1, 0].tolist() == [50.0, 49.0, 48.0]
    assert flat['gt_num_keypoints'].tolist() == [[4, 0, 0], [0, 0, 0], [17, 0, 0]] and not flat['gt_keypoints'][1].any()
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations([[_ann(None, 3)]], (20, 20), 3, keypoints=True)              # no 'keypoints'
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations([[_ann(kps, None)]], (20, 20), 3, keypoints=True)            # no 'num_keypoints'
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations([[_ann(kps, 3), _ann(kps[:48], 3)]], (20, 20), 3, keypoints=True)    # another Kp
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations([[]], (20, 20), 3, keypoints=True)                           # Kp unknown
    assert coco_gt.flatten_annotations([[]], (20, 20), 3, keypoints=True, num_keypoints=17)['gt_keypoints'].shape == (1, 3, 17, 3)
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations([[_ann(kps, 3)]], (20, 20), 3, keypoints=True, num_keypoints=16)     # 51 values, 48 expected
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations([[]], (20, 20), 3, num_keypoints=17)                         # without keypoints=True
