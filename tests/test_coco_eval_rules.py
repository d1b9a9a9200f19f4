"""tests/coco_eval_np.py (the numpy restatement of the COCO evaluation rules in include/scda_ops.h) against the arrays recorded from the
reference's own cocoeval.py / maskApi.c in tests/golden/coco_eval_ref.npz.  No GPU."""
import os

import numpy as np
import pytest

import coco_eval_np as cnp
from conftest import ROOT

SETS = ('rules', 'random_bbox', 'random_segm')
_CACHE = {}


def fixture():
    if 'z' not in _CACHE:
        _CACHE['z'] = dict(np.load(os.path.join(ROOT, "tests", "golden", "coco_eval_ref.npz")))
    return _CACHE['z']


def evaluated(name):
    """(images, K, params, coco_eval_np's result), computed once per set and not modified"""
    if name not in _CACHE:
        images, K, params = cnp.load_set(fixture(), name)
        _CACHE[name] = (images, K, params, cnp.evaluate(images, K, params))
    return _CACHE[name]


def test_parameters_are_the_references_defaults():
    p = cnp.default_params()
    assert len(p['iou_thrs']) == 10 and p['iou_thrs'][0] == 0.5 and len(p['rec_thrs']) == 101 and p['max_dets'] == [1, 10, 100]
    assert np.array_equal(fixture()['rules_area_rng'], p['area_rng'])
    assert cnp.stat_specs(p['iou_thrs'], p['max_dets'])[:3, 1].tolist() == [-1, 0, 5]


def test_bb_iou_equals_the_references():
    z = fixture()
    for name in ('rules', 'random_bbox'):
        for im in cnp.load_set(z, name)[0]:
            if im['iou'].size:
                assert np.array_equal(cnp.bb_iou(im['dt_xywh'], im['gt_xywh'], im['gt_iscrowd']), im['iou'])
    assert (z['rules_iou'] == 0.5).any()


@pytest.mark.parametrize("name", SETS)
def test_matching_equals_the_recorded_eval_imgs(name):
    z = fixture()
    images, K, params, res = evaluated(name)
    max_det = params['max_dets'][-1]
    rank = np.concatenate([e['rank'] for e in res['per_image']])
    part = z[name + '_rank'] >= 0
    assert np.array_equal(rank[part], z[name + '_rank'][part]) and (rank[~part] >= max_det).all()
    assert np.array_equal(np.concatenate([e['match'] for e in res['per_image']]), z[name + '_match'])
    assert np.array_equal(np.concatenate([e['ignore'] for e in res['per_image']]).astype(np.uint8), z[name + '_ignore'])
    assert np.array_equal(np.concatenate([e['gt_ignore'] for e in res['per_image']]).astype(np.uint8), z[name + '_gt_ignore'])
    assert np.array_equal(sum(e['npig'] for e in res['per_image']), z[name + '_npig'])


@pytest.mark.parametrize("name", SETS)
def test_accumulate_equals_the_recorded_eval(name):
    z = fixture()
    res = evaluated(name)[3]
    for key in ('precision', 'recall', 'scores'):
        assert res[key].dtype == np.float64 and np.array_equal(res[key], z[name + '_' + key]), key


@pytest.mark.parametrize("name", SETS)
def test_stats_within_the_summation_bound(name):
    z = fixture()
    res = evaluated(name)[3]
    n = cnp.stat_counts(res['precision'], res['recall'], res['specs'])
    assert np.all(np.abs(res['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53), (res['stats'], z[name + '_stats'])
    assert ((z[name + '_stats'] == -1) == (n == 0)).all()
