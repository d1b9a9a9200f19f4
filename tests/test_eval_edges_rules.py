"""The structural edge sets of the two evaluators (tests/eval_edge_cases.py) on the CPU: the numpy statements (coco_eval_np.evaluate,
voc_map_np.evaluate / recall) against the arrays the reference's own code recorded for them in tests/golden/coco_eval_ref.npz and
voc_map_ref.npz, bit for bit, and -- from the inputs -- that every set still crosses the boundary of scda_amd/csrc/coco_eval.hip,
map_eval.hip, radix_sort.h or eval_prims.h (block_scan256, wave_compact) it was built for, so that a case that stops crossing it fails
here and does not pass quietly on the GPU.  The constants named below are the kernels'.  No GPU."""
import hashlib

import numpy as np
import pytest

import coco_eval_np as cnp
import eval_edge_cases as edges
import voc_map_np as vnp
from test_coco_eval_rules import fixture as coco_fixture
from test_voc_map_rules import fixture as map_fixture

K_MATCH_THREADS, K_IOU_LDS, K_SORT_TILE, K_MAX_PER = 128, 2048, 1024, 1024   # coco_eval.hip, radix_sort.h
_CACHE = {}


def coco_evaluated(name):
    """(images, K, params, coco_eval_np's result) of an edge set, computed once and not modified"""
    if ('coco', name) not in _CACHE:
        images, K, params = edges.load_coco_set(coco_fixture(), name)
        _CACHE['coco', name] = (images, K, params, cnp.evaluate(images, K, params))
    return _CACHE['coco', name]


def map_evaluated(name):
    """(images, C, sum_gt, voc_map_np's result) of an edge set, computed once and not modified"""
    if ('map', name) not in _CACHE:
        z = map_fixture()
        images, C, sum_gt = vnp.load_set(z, name)
        _CACHE['map', name] = (images, C, sum_gt, vnp.evaluate(images, C, sum_gt=sum_gt, keep_num=int(z[name + '_keep_num'])))
    return _CACHE['map', name]


def _digest(z, sets):
    h = hashlib.sha256()
    for k in sorted(z):
        if any(k.startswith(s + '_') for s in sets):
            a = z[k]
            for part in (k.encode(), str(a.dtype).encode(), str(a.shape).encode(), a.tobytes()):
                h.update(part)
    return h.hexdigest()


def test_the_older_sets_are_byte_identical():
    """name, type, shape and bytes of every array of the sets that were there before the edge sets were added"""
    assert _digest(coco_fixture(), ('rules', 'random_bbox', 'random_segm')) == 'ea6930b86a139b7b0b29a5542941ba1269eea92b24333643ee65eca127553dd5'
    assert _digest(map_fixture(), ('rules', 'nan', 'random')) == '50d571d0d2a2b27fc37392a39093564035a5862d2318dca82babf11fd1be8710'
    assert sum(not any(k.startswith(s + '_') for s in edges.COCO_SETS) for k in coco_fixture()) == 72
    assert sum(not any(k.startswith(s + '_') for s in edges.MAP_SETS) for k in map_fixture()) == 57


# ------------------------------------------------------------------------------------------------ COCO
@pytest.mark.parametrize("name", edges.COCO_SETS)
def test_coco_builders_give_the_recorded_inputs(name):
    case, (images, K, params, _) = edges.coco_case(name), coco_evaluated(name)
    assert K == case['K'] and len(images) == len(case['images'])
    for key in ('iou_thrs', 'rec_thrs', 'area_rng'):
        assert np.asarray(params[key]).tobytes() == np.asarray(case['params'][key], dtype=np.float64).tobytes(), key
    assert params['max_dets'] == list(case['params']['max_dets'])
    for got, want in zip(images, case['images']):
        assert got['image_id'] == want['image_id']
        for key in ('dt_corners', 'dt_score', 'dt_cat', 'gt_xywh', 'gt_area', 'gt_iscrowd', 'gt_cat'):
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
        assert max(len(got['dt_score']), 1) <= case['D'] and max(len(got['gt_cat']), 1) <= case['G']


@pytest.mark.parametrize("name", edges.COCO_SETS)
def test_coco_statement_equals_the_recorded_arrays(name):
    z = coco_fixture()
    images, K, params, res = coco_evaluated(name)
    rank = np.concatenate([e['rank'] for e in res['per_image']])
    part = z[name + '_rank'] >= 0
    assert np.array_equal(rank[part], z[name + '_rank'][part]) and (rank[~part] >= params['max_dets'][-1]).all()
    assert np.array_equal(np.concatenate([e['match'] for e in res['per_image']]), z[name + '_match'])
    assert np.array_equal(np.concatenate([e['ignore'] for e in res['per_image']]).astype(np.uint8), z[name + '_ignore'])
    assert np.array_equal(np.concatenate([e['gt_ignore'] for e in res['per_image']]).astype(np.uint8), z[name + '_gt_ignore'])
    assert np.array_equal(sum(e['npig'] for e in res['per_image']), z[name + '_npig'])
    for key in ('precision', 'recall', 'scores'):
        assert res[key].dtype == z[name + '_' + key].dtype == np.float64 and res[key].tobytes() == z[name + '_' + key].tobytes(), key
    n = cnp.stat_counts(res['precision'], res['recall'], res['specs'])
    assert np.all(np.abs(res['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53), (res['stats'], z[name + '_stats'])
    assert ((z[name + '_stats'] == -1) == (n == 0)).all()


def _per_category(im, K, max_det):
    """[(Dc, Gc, Dm)] of one image, category 1..K"""
    return [(int((im['dt_cat'] == k).sum()), int((im['gt_cat'] == k).sum()), min(int((im['dt_cat'] == k).sum()), max_det)) for k in range(1, K + 1)]


def test_waves_crosses_the_match_kernels_rounds():
    images, K, params, res = coco_evaluated('waves')
    per = _per_category(images[0], K, params['max_dets'][-1])
    assert [(d, g) for d, g, _ in per] == [(32, 64), (33, 64), (64, 65), (0, 5), (128, 6), (129, 6)]
    assert per[0][1] == 64 and per[2][1] == 65                               # one round of wave_compact and two claim words; one more of each
    assert per[4][0] == K_MATCH_THREADS and per[5][0] == K_MATCH_THREADS + 1
    assert per[0][1] * per[0][2] == K_IOU_LDS and K_IOU_LDS < per[1][1] * per[1][2] == 64 * 33                # staged beside not staged
    assert [dm for _, _, dm in per] == [32, 33, 64, 0, 100, 100]             # the 32-detection flush: full, one over, two full, none
    assert per[3][1] > 0 and per[3][0] == 0
    rank = res['per_image'][0]['rank']
    assert (rank >= 100).sum() == 28 + 29 and (res['per_image'][0]['match'][rank >= 100] == -1).all()         # the tail loop
    m = res['per_image'][0]['match']
    assert all((m[images[0]['dt_cat'] == k] >= 0).any() for k in (1, 2, 3, 5, 6))
    assert np.unique(np.diff(np.flatnonzero(images[0]['gt_cat'] == 3))).size > 1                             # the lists are not contiguous


def test_capacity_fills_the_lists_and_the_claim_words():
    images, K, params, res = coco_evaluated('capacity')
    case = edges.coco_case('capacity')
    assert case['D'] == case['G'] == K_MAX_PER
    assert len(images[0]['dt_score']) == K_MAX_PER and (images[0]['dt_cat'] == 1).all()
    gl = np.flatnonzero(images[1]['gt_cat'] == 2)
    assert len(images[1]['gt_cat']) == K_MAX_PER and len(gl) == 1000 and (len(gl) + 31) // 32 == K_MAX_PER // 32      # every word of s_gtm
    crowd_at = np.flatnonzero(images[1]['gt_iscrowd'][gl])
    assert len(crowd_at) == 80 and crowd_at.max() >= 992 and (crowd_at >= 512).sum() > 10                   # bit 15 beside a large position
    assert len(gl) * min(int((images[1]['dt_cat'] == 2).sum()), 100) > K_IOU_LDS
    assert max(int((images[1]['gt_cat'] == k).sum()) for k in (1, 3)) <= 24                                 # the other categories stay small
    assert len(images[2]['dt_score']) == 0 and len(images[2]['gt_cat']) > 0
    assert len(images[3]['gt_cat']) == 0 and len(images[3]['dt_score']) > 0
    assert (len(images) * case['D']) % K_SORT_TILE == 0
    # the greedy matching reaches list positions >= 512 (rows of the image -> positions in the category's list), crowds among them
    m = res['per_image'][1]['match'][images[1]['dt_cat'] == 2]
    pos = np.searchsorted(gl, m[m >= 0])
    assert pos.max() >= 512 and images[1]['gt_iscrowd'][m[m >= 0]].any()


@pytest.mark.parametrize("name", ('limits', 'limits3'))
def test_limits_run_the_documented_parameter_limits(name):
    z = coco_fixture()
    images, K, params, res = coco_evaluated(name)
    T, R, A, M = len(params['iou_thrs']), len(params['rec_thrs']), len(params['area_rng']), len(params['max_dets'])
    assert (T, R, A) == (16, 128, 8) and M == (4 if name == 'limits' else 3)
    assert T * A == K_MATCH_THREADS                                          # every lane of the matcher is active
    thr = params['iou_thrs']
    assert thr[-1] == 1.0 and .5 not in thr and .75 not in thr
    assert (z[name + '_match'][:, 0, T - 1] >= 0).any(), "a match at the threshold clamped to 1 - 1e-10"
    assert res['specs'][1, 1] == res['specs'][2, 1] == -2 and z[name + '_stats'][1] == z[name + '_stats'][2] == -1
    assert (z[name + '_npig'][:, 7] == 0).all() and (z[name + '_precision'][..., 7, :] == -1).all()          # an area range nothing is in
    most = max(d for im in images for d, _, _ in _per_category(im, K, 10 ** 6))
    if name == 'limits':
        assert params['max_dets'] == [1, 5, 20, 100] and res['specs'][0].tolist() == [1, -1, 0, 3] and set(res['specs'][1:6, 3]) == {2}
        assert res['specs'][6:, 3].tolist() == [0, 1, 2, 2, 2, 2] and z[name + '_stats'][0] > 0
    else:
        assert 100 not in params['max_dets'] and res['specs'][0, 1] == -2 and z[name + '_stats'][0] == -1 and (z[name + '_stats'][3:] > -1).all()
        assert most > params['max_dets'][-1]                                 # ranks past maxDets[-1] = 30
    assert 64 <= len(images) * edges.coco_case(name)['D'] < K_SORT_TILE


def test_sortkeys_crosses_every_branch_of_the_keys():
    images, K, params, res = coco_evaluated('sortkeys')
    ids = [im['image_id'] for im in images]
    assert ids == sorted(ids, reverse=True) and min(ids) < 0 and max(ids) >= 2 ** 24                        # added in descending id order
    sc = np.concatenate([im['dt_score'] for im in images])
    tiny = np.finfo(np.float32).tiny
    assert (sc < 0).any() and ((sc == 0) & ~np.signbit(sc)).any() and ((sc == 0) & np.signbit(sc)).any() and ((sc > 0) & (sc < tiny)).any()
    assert K == 255 and set(np.concatenate([im['dt_cat'] for im in images])) == {1, 255}
    assert len(images) * edges.coco_case('sortkeys')['D'] < 64
    # equal scores in all three images, and the tie is visible: the tied rows are not all matched or all unmatched
    for k, s in ((1, 0.5), (1, -0.25), (1, 0.0), (255, 0.5)):
        hit = [e['match'][(im['dt_cat'] == k) & (im['dt_score'] == np.float32(s)), 0, 0] >= 0 for im, e in zip(images, res['per_image'])]
        assert all(len(h) for h in hit) and len({tuple(h) for h in hit}) > 1, (k, s)
    # by image id, not by add order: the statement over the images in ascending order gives the same bytes
    again = cnp.evaluate(images[::-1], K, params)
    assert all(again[key].tobytes() == res[key].tobytes() for key in ('precision', 'recall', 'scores'))
    by_add_order = cnp.evaluate([dict(im, image_id=i) for i, im in enumerate(images)], K, params)           # ids ascending as added
    assert by_add_order['precision'].tobytes() != res['precision'].tobytes(), "resolving the ties in add order must show"
    assert (res['scores'] < 0).any()


def test_prrounds_crosses_the_256_row_rounds():
    images, K, params, res = coco_evaluated('prrounds')
    rows = [sum(_per_category(im, K, params['max_dets'][-1])[k][2] for im in images) for k in range(K)]
    assert rows == [256, 257, 600] and rows[2] > 512
    assert [tuple(_per_category(im, K, 10 ** 6)[k][0] for im in images) for k in range(K)] == [edges.PR_ROWS[k] for k in (1, 2, 3)]
    assert params['max_dets'] == [1, 10, 100]                                # rank < 1 and rank < 10 drop rows inside every round
    assert (res['recall'][0, :, 0, 0] < res['recall'][0, :, 0, 1]).all() and (res['recall'][0, :, 0, 1] < res['recall'][0, :, 0, 2]).all()


# ------------------------------------------------------------------------------------------------ Cityscapes mAP
@pytest.mark.parametrize("name", edges.MAP_SETS)
def test_map_builders_give_the_recorded_inputs(name):
    built, _, C = edges.map_case(name)
    images, C2, _, _ = map_evaluated(name)
    caps = edges.MAP_CAPS[name]
    assert C == C2 and len(images) == len(built) and int(map_fixture()[name + '_keep_num']) == caps['keep_num'] <= caps['D']
    for got, want in zip(images, built):
        assert got['name'] == want['name']
        for key in ('det', 'info', 'gt') + (('props', 'rgts') if 'props' in want else ()):
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
        assert len(got['det']) <= caps['D'] and len(got['gt']) <= caps['G']


@pytest.mark.parametrize("name", edges.MAP_SETS)
def test_map_statement_equals_the_recorded_arrays(name):
    z = map_fixture()
    images, C, sum_gt, res = map_evaluated(name)
    got, score = [], []
    for c in range(1, C):
        for i, e in enumerate(res['per_image']):
            for d in e['order'][e['cls'][e['order']] == c]:
                got.append([c, i] + e['box'][d].tolist()); score.append(float(str(e['score'][d])))
    assert np.array_equal(np.asarray(got, dtype=np.int32).reshape(-1, 6), z[name + '_res'])
    assert np.asarray(score).tobytes() == z[name + '_res_score'].tobytes()
    assert np.array_equal(res['rows'], np.bincount(z[name + '_res'][:, 0], minlength=C))
    assert np.array_equal(np.concatenate([e['tp'] for e in res['per_image']]), z[name + '_tp'])
    assert np.array_equal(np.concatenate([e['match'] for e in res['per_image']]), z[name + '_match'])
    assert np.array_equal(np.concatenate([e['claimed'] for e in res['per_image']]), z[name + '_is_det'])
    for key in ('ap', 'max_recall'):
        assert np.array_equal(res[key], z[name + '_' + key], equal_nan=True), key
        fin = np.isfinite(res[key])
        assert res[key][fin].tobytes() == z[name + '_' + key][fin].tobytes(), key
    assert np.array_equal(res['mAP'], z[name + '_mAP'], equal_nan=True)
    assert (res['rows'][1:] > 0).all(), "the reference is asked about every class, and raises on one without a row"


@pytest.mark.parametrize("name", ('cap', 'keep100'))
def test_cap_crosses_the_row_and_scan_rounds(name):
    z = map_fixture()
    images, C, sum_gt, res = map_evaluated(name)
    caps = edges.MAP_CAPS[name]
    assert [len(im['det']) for im in images] == [256, 257, 1024] and caps['D'] == 1024                      # map_rows_kernel: 1, 2 and 4 rounds of 256
    det = np.concatenate([im['det'] for im in images])
    assert np.bincount(det[:, 6].astype(np.int64), minlength=10).tolist() == [edges.CAP_CLASS_ROWS.get(c, 0) for c in range(10)]
    if name == 'cap':
        assert caps['keep_num'] == caps['D'] and res['rows'].tolist() == [0, 256, 257, 1000, 8, 6]          # map_pr_kernel: 256, 257, > 512 rows
    else:
        assert caps['keep_num'] == 100 and all(int((e['rank'] < 100).sum()) == 100 for e in res['per_image'])
        assert res['rows'].sum() == sum(int(e['kept'].sum()) for e in res['per_image']) <= 300
    assert sum_gt[4] > 0 and (z[name + '_tp'][det[:, 6] == 4] == 0).all() and z[name + '_ap'][4] == 0 and res['rows'][4] > 0      # all false positives
    assert sum_gt[5] == 0 and res['rows'][5] > 0 and np.isnan(z[name + '_ap'][5]) and np.isnan(z[name + '_max_recall'][5])
    assert all(0 < z[name + '_ap'][c] < 1 for c in (1, 2, 3))
    sc = det[:, 5]
    assert (sc < 0).any() and ((sc == 0) & ~np.signbit(sc)).any() and ((sc == 0) & np.signbit(sc)).any()
    # ties inside an image and across the images, within one class
    for c in (1, 2, 3):
        per = [im['det'][im['det'][:, 6] == c, 5] for im in images]
        assert any(len(np.unique(p)) < len(p) for p in per) and len(set(per[0]) & set(per[1]) & set(per[2])) > 0
    assert (det[:, 1] < 0).any() and (det[:, 1:5] != np.trunc(det[:, 1:5])).any()                           # the clip and the truncation


def test_match_crosses_the_wave_rounds_and_the_class_limit():
    z = map_fixture()
    images, C, sum_gt, res = map_evaluated('match')
    by = {im['name']: (im, e) for im, e in zip(images, res['per_image'])}
    assert C == 256 and res['rows'][1] > 1 and res['rows'][255] > 1 and sum_gt[1] > 0 and sum_gt[255] > 0 and (res['rows'][1:] > 0).all()
    assert z['match_ap'][1] > 0 and z['match_ap'][255] > 0
    count = lambda n, c: int((by[n][0]['gt'][:, 4] == c).sum())               # noqa: E731
    assert count('g64', 1) == 64 and count('g65', 255) == 65 and count('g1000', 7) == 1000 and len(by['g1000'][0]['gt']) == K_MAX_PER
    # g64: the last of 64, the first, nothing overlaps, only touching
    im, e = by['g64']
    assert e['match'][:4].tolist() == [63, 0, -1, -1] and vnp.best_iou(e['box'][2], im['gt'][:64]) == (-1, -1) == vnp.best_iou(e['box'][3], im['gt'][:64])
    assert e['match'][4:].tolist() == [64, -1] and (im['gt'][64:, :4] == im['gt'][64, :4]).all()              # three equal boxes: the first, then taken
    # g65: the boxes at the class's indices 63 and 64 are one box, on both sides of the wave round
    im, e = by['g65']
    rows = np.flatnonzero(im['gt'][:, 4] == 255)
    assert (im['gt'][rows[63], :4] == im['gt'][rows[64], :4]).all() and np.diff(rows).max() > 1
    assert e['match'].tolist() == [rows[63], -1, -1, rows[10], int(np.flatnonzero(im['gt'][:, 4] == 3)[0])] and not e['claimed'][rows[64]]
    # g1000: one box at j, j + 1, j + 64; the halfway detections
    im, e = by['g1000']
    rows = np.flatnonzero(im['gt'][:, 4] == 7)
    for j in edges.MATCH_DUPS:
        assert (im['gt'][rows[[j + 1, j + 64]], :4] == im['gt'][rows[j], :4]).all()
        same = np.flatnonzero((im['det'][:, 1:5] == im['gt'][rows[j], :4]).all(1))
        same = same[np.argsort(-im['det'][same, 5])]
        assert len(same) == 3 and e['match'][same].tolist() == [rows[j], -1, -1] and not e['claimed'][rows[[j + 1, j + 64]]].any()
        assert vnp.best_iou(e['box'][same[1]], im['gt'][rows]) == (1.0, j)
    assert max(edges.MATCH_DUPS) + 64 >= 512 and 63 in edges.MATCH_STRADDLE and 511 in edges.MATCH_STRADDLE
    for j in edges.MATCH_STRADDLE:
        box = np.asarray(edges.match_gt(j)) + (6, 0, 6, 0)
        d = int(np.flatnonzero((im['det'][:, 1:5] == box).all(1))[0])
        iou = [vnp.best_iou(box, im['gt'][rows[[q]]])[0] for q in (j, j + 1)]
        assert iou[0] == iou[1] == 14 / 26 and vnp.best_iou(box, im['gt'][rows]) == (14 / 26, j) and e['match'][d] == rows[j]
    far = int(np.flatnonzero((im['det'][:, 1:5] == (850, 650, 880, 690)).all(1))[0])
    assert vnp.best_iou(e['box'][far], im['gt'][rows]) == (-1, -1) and e['match'][far] == -1


def test_recall_crosses_the_wave_and_row_strides():
    z = map_fixture()
    images, C, _, res = map_evaluated('recall')
    caps = edges.MAP_CAPS['recall']
    assert [(len(im['props']), len(im['rgts'])) for im in images] == list(edges.RECALL_SHAPES) and caps['P'] > 64
    assert sorted(p for p, _ in edges.RECALL_SHAPES) == [0, 64, 64, 65, 200] and sorted(r for _, r in edges.RECALL_SHAPES) == [0, 1, 4, 5, 9]
    each = [vnp.recall(im['props'], im['rgts']) for im in images]
    assert np.array_equal(np.asarray(each), z['recall_recalled_each'])
    assert (res['rpn_recalled'], res['rpn_gts']) == (int(z['recall_recalled']), int(z['recall_rpn_gts'])) == tuple(np.sum(each, 0))
    assert 0 < res['rpn_recalled'] < res['rpn_gts']
    # the only overlapping proposal of a row sits at index 64 / 150, and the row is recalled through it
    for i, row, at in ((2, 0, 64), (3, 8, 150)):
        ov = vnp.overlaps_f32(images[i]['rgts'], images[i]['props'][:, 1:5])
        assert np.flatnonzero(ov[row] > 0).tolist() == [at] and ov[row, at] > 0.5
        cut = np.delete(images[i]['props'], at, 0)
        assert vnp.recall(cut, images[i]['rgts'])[0] == each[i][0] - 1
    ov = vnp.overlaps_f32(images[3]['rgts'], images[3]['props'][:, 1:5])
    assert ov.dtype == np.float32 and ov[4].max() == np.float32(0.5) and np.flatnonzero(ov[4] > 0).tolist() == [7]     # exactly 0.5: not recalled
