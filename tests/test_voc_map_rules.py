"""tests/voc_map_np.py (the numpy restatement of the Cityscapes mAP rules R1..R4 in include/scda_ops.h) against the arrays recorded from
the reference's own utils/cal_mAP.py and compute_recall in tests/golden/voc_map_ref.npz and in the two eval_*.npz of the evaluation
path, and scda_amd.evaluate.meta_ground_truth against the project's parse_gts.  No GPU."""
import os

import numpy as np
import pytest

import voc_map_np as vnp
from conftest import GOLDEN

SETS = ('rules', 'nan', 'random')
EVAL_FILES = ('eval_256x512', 'eval_512x1024')
NUM_CLASSES_EVAL = 9
_CACHE = {}


def fixture():
    if 'z' not in _CACHE:
        _CACHE['z'] = dict(np.load(os.path.join(GOLDEN, "voc_map_ref.npz")))
    return _CACHE['z']


def evaluated(name):
    """(images, C, sum_gt, voc_map_np's result), computed once per set and not modified"""
    if name not in _CACHE:
        images, C, sum_gt = vnp.load_set(fixture(), name)
        _CACHE[name] = (images, C, sum_gt, vnp.evaluate(images, C, sum_gt=sum_gt))
    return _CACHE[name]


def eval_case(file, tag):
    """the synth rows of an eval_*.npz as images for the rules (parsed back to float32, scale 1, in file order) -> (images, ground truth
    of meta_ground_truth, the recorded ap / max_recall / mAP)"""
    from scda_amd import evaluate
    key = (file, tag)
    if key not in _CACHE:
        z = np.load(os.path.join(GOLDEN, file + ".npz"))
        gt = evaluate.meta_ground_truth(str(z['meta' + tag]).splitlines(True), NUM_CLASSES_EVAL)
        images = vnp.parse_text_rows(str(z['synth_results' + tag]))
        for im in images:
            assert len(im['det']) <= 100 and (im['det'][:, 1:5] >= 0).all() and (im['det'][:, 1:5] <= 4095).all()
            im['info'] = np.asarray([4096, 4096, 1.0], dtype=np.float32)      # no coordinate is clipped: the rows were written clipped
            im['gt'] = gt.get(im['name'], np.zeros((0, 5), dtype=np.int32))
        _CACHE[key] = (images, gt, z['ap_synth' + tag], z['max_recall_synth' + tag], z['mAP_synth' + tag])
    return _CACHE[key]


@pytest.mark.parametrize("name", SETS)
def test_rows_equal_what_the_reference_parsed(name):
    z = fixture()
    images, C, _, res = evaluated(name)
    got, score = [], []
    for c in range(1, C):
        for i, e in enumerate(res['per_image']):
            for d in e['order'][e['cls'][e['order']] == c]:
                got.append([c, i] + e['box'][d].tolist()); score.append(float(str(e['score'][d])))
    assert np.array_equal(np.asarray(got, dtype=np.int32).reshape(-1, 6), z[name + '_res'])
    assert np.array_equal(np.asarray(score), z[name + '_res_score'])
    assert np.array_equal(res['rows'], np.bincount(z[name + '_res'][:, 0], minlength=C))


@pytest.mark.parametrize("name", SETS)
def test_matching_and_ap_equal_the_recorded(name):
    z = fixture()
    images, C, sum_gt, res = evaluated(name)
    assert np.array_equal(np.concatenate([e['tp'] for e in res['per_image']]), z[name + '_tp'])
    assert np.array_equal(np.concatenate([e['match'] for e in res['per_image']]), z[name + '_match'])
    assert np.array_equal(np.concatenate([e['claimed'] for e in res['per_image']]), z[name + '_is_det'])
    assert res['ap'].tobytes() == z[name + '_ap'].tobytes() or np.isnan(z[name + '_ap']).any()
    assert np.array_equal(res['ap'], z[name + '_ap'], equal_nan=True) and np.array_equal(res['max_recall'], z[name + '_max_recall'], equal_nan=True)
    assert np.array_equal(res['mAP'], z[name + '_mAP'], equal_nan=True)
    if name == 'nan':
        assert np.isnan(res['ap'][2]) and np.isnan(res['max_recall'][2]) and not np.isnan(res['ap'][1])
    if z[name + '_in_meta'].all() and name != 'rules':                       # every meta image is added: the counted sum is the meta's
        assert np.array_equal(vnp.evaluate(images, C)['sum_gt'], sum_gt)


def test_recall_equals_the_recorded():
    z = fixture()
    res = evaluated('random')[3]
    assert (res['rpn_recalled'], res['rpn_gts']) == (int(z['random_recalled']), int(z['random_rpn_gts']))
    assert vnp.recall(np.zeros((0, 6), np.float32), np.ones((3, 5), np.float32)) == (0, 3)


@pytest.mark.parametrize("file", EVAL_FILES)
@pytest.mark.parametrize("tag", ["", "3"])
def test_eval_path_rows_give_the_recorded_ap(file, tag):
    images, gt, ap, max_recall, m = eval_case(file, tag)
    res = vnp.evaluate(images, NUM_CLASSES_EVAL, sum_gt=gt['num'])
    assert np.array_equal(res['ap'], ap, equal_nan=True) and np.array_equal(res['max_recall'], max_recall, equal_nan=True)
    assert np.array_equal(res['mAP'], m, equal_nan=True)


@pytest.mark.parametrize("file", EVAL_FILES)
@pytest.mark.parametrize("tag", ["", "3"])
def test_meta_ground_truth_equals_parse_gts(file, tag):
    from scda_amd import evaluate
    from scda_amd.dropin.utils.cal_mAP import parse_gts
    lines = str(np.load(os.path.join(GOLDEN, file + ".npz"))['meta' + tag]).splitlines(True)
    want, got = parse_gts(lines, NUM_CLASSES_EVAL), evaluate.meta_ground_truth(lines, NUM_CLASSES_EVAL)
    names = [k for k in want if k != 'num']
    assert sorted(names) == sorted(k for k in got if k != 'num') and len(names) >= 2
    assert np.array_equal(got['num'], want['num']) and got['num'].sum() > 0
    for k in names:
        assert got[k].dtype == np.int32 and len(got[k]) == want[k]['bbox_num']
        for c in range(1, NUM_CLASSES_EVAL):
            assert got[k][got[k][:, 4] == c][:, :4].tolist() == want[k]['bbox'][c]


def test_meta_ground_truth_ignores_labels_outside_the_classes(tmp_path):
    from scda_amd import evaluate
    text = "# 0\nval/c/a_leftImg8bit.png\n3\n10\n20\n0\n0\n4\n0 1 2 3 4\n2 5 6 7 8\n5 1 1 2 2\n2 0 0 9 9\n# 1\nval/c/b.png\n3\n10\n20\n0\n0\n0\n"
    p = tmp_path / "meta.txt"
    p.write_text(text)
    for src in (str(p), text.splitlines(True)):
        gt = evaluate.meta_ground_truth(src, 5)
        assert gt['num'].tolist() == [0, 0, 2, 0, 0]
        assert gt['a_leftImg8bit'].tolist() == [[1, 2, 3, 4, 0], [5, 6, 7, 8, 2], [1, 1, 2, 2, 5], [0, 0, 9, 9, 2]] and gt['b'].shape == (0, 5)
