"""The COCO AP and Cityscapes mAP kernels (scda_amd/csrc/coco_eval.hip, map_eval.hip, radix_sort.h) at their structural edges on the
MI355X: CocoEvaluator and MapEvaluator over the edge sets of tests/eval_edge_cases.py, against the arrays the reference's own code
recorded for them (tests/golden/coco_eval_ref.npz, voc_map_ref.npz) and against the numpy statements (coco_eval_np, voc_map_np), plus
native.coco_box_iou and native.map_recall called directly.  Everything is compared bit for bit; the one exception are the 12 COCO
stats, whose bound 2 n 2^-53 between two summation orders is the one test_coco_eval_gpu.py derives.  tests/test_eval_edges_rules.py
asserts, without a GPU, the boundary every set crosses."""
import numpy as np
import pytest
import torch

import coco_eval_np as cnp
import eval_edge_cases as edges
import voc_map_np as vnp
from test_coco_eval_gpu import _batch as _coco_batch, _dev
from test_coco_eval_rules import fixture as coco_fixture
from test_eval_edges_rules import coco_evaluated, map_evaluated
from test_voc_map_gpu import _collect
from test_voc_map_rules import fixture as map_fixture

pytestmark = pytest.mark.gpu

_RUNS = {}


# ------------------------------------------------------------------------------------------------ COCO
def _coco_run(name, cuda, order=None, batch=None, debug=True):
    """the set through a CocoEvaluator of the set's capacities and parameters -> host arrays, per-detection ones in the fixture's order"""
    from scda_amd.coco_eval import CocoEvaluator
    images, K, params, _ = coco_evaluated(name)
    D, G = edges.COCO_CAPS[name]
    order = list(range(len(images))) if order is None else list(order)
    batch = len(images) if batch is None else batch
    ev = CocoEvaluator(K, 'bbox', max_images=len(images), max_dets_per_image=D, max_gts_per_image=G, device=cuda, params=params, debug=debug)
    for s in range(0, len(order), batch):
        ev.add(*_coco_batch(images, order[s:s + batch], D, G, cuda)[0])
    res = {k: v.cpu().numpy().copy() for k, v in ev.accumulate().items()}
    res['stats'] = ev.summarize()
    res['npig'], res['seen'] = ev.npig.cpu().numpy(), ev.seen.cpu().numpy()
    slot = {i: s for s, i in enumerate(order)}
    pick = lambda t: np.concatenate([t[slot[i], :len(images[i]['dt_score'])] for i in range(len(images))])   # noqa: E731
    res['rank'], res['bits'] = pick(ev.rank.cpu().numpy()), pick(ev.bits.cpu().numpy().view(np.uint32))
    if debug:
        res['match'] = pick(ev.debug_match.cpu().numpy())
    return res


def _coco_default(name, cuda):
    if ('coco', name) not in _RUNS:
        _RUNS['coco', name] = _coco_run(name, cuda)
    return _RUNS['coco', name]


@pytest.mark.parametrize("name", edges.COCO_SETS)
def test_coco_matching_equals_the_recorded_and_the_statement(cuda, name):
    z = coco_fixture()
    images, K, params, res = coco_evaluated(name)
    got = _coco_default(name, cuda)
    T, last = len(params['iou_thrs']), params['max_dets'][-1]
    part = z[name + '_rank'] >= 0
    assert np.array_equal(got['rank'][part], z[name + '_rank'][part]) and (got['rank'][~part] >= last).all()
    assert np.array_equal(got['rank'], np.concatenate([e['rank'] for e in res['per_image']]))
    assert np.array_equal(got['match'], z[name + '_match']) and np.array_equal(got['match'], np.concatenate([e['match'] for e in res['per_image']]))
    t = np.arange(T)
    matched, ignored = (got['bits'][:, :, None] >> t) & 1, (got['bits'][:, :, None] >> (16 + t)) & 1
    assert np.array_equal(matched, (z[name + '_match'] >= 0).astype(np.uint32))
    assert np.array_equal(ignored, z[name + '_ignore'].astype(np.uint32))
    used = np.uint32(((1 << T) - 1) * 0x10001)
    assert not (got['bits'] & ~used).any()                                   # nothing beyond the T thresholds of either half
    assert np.array_equal(got['npig'], z[name + '_npig']) and np.array_equal(got['npig'], sum(e['npig'] for e in res['per_image']))
    assert np.array_equal(got['seen'] != 0, np.logical_or.reduce([e['seen'] for e in res['per_image']]))


@pytest.mark.parametrize("name", edges.COCO_SETS)
def test_coco_accumulate_is_bit_equal_and_stats_within_the_bound(cuda, name):
    z = coco_fixture()
    res = coco_evaluated(name)[3]
    got = _coco_default(name, cuda)
    for key in ('precision', 'recall', 'scores'):
        want = z[name + '_' + key]
        assert got[key].dtype == np.float64 and got[key].shape == want.shape
        assert got[key].tobytes() == want.tobytes(), (key, int((got[key] != want).sum()))
        assert got[key].tobytes() == res[key].tobytes(), key
    n = cnp.stat_counts(z[name + '_precision'], z[name + '_recall'], res['specs'])
    print(name, "stats", got['stats'], "max |diff|", np.abs(got['stats'] - z[name + '_stats']).max())
    assert np.all(np.abs(got['stats'] - z[name + '_stats']) <= 2.0 * n * 2.0 ** -53), (got['stats'], z[name + '_stats'])
    assert np.all(np.abs(got['stats'] - res['stats']) <= 2.0 * n * 2.0 ** -53), (got['stats'], res['stats'])
    assert ((got['stats'] == -1) == (z[name + '_stats'] == -1)).all()


@pytest.mark.parametrize("name", ('sortkeys', 'limits3', 'prrounds'))
def test_coco_order_and_batching_of_the_images_do_not_matter(cuda, name):
    """ties go by image id, never by the order of the add() calls: ascending order and single-image batches give the same bytes"""
    base = _coco_default(name, cuda)
    n = len(coco_evaluated(name)[0])
    for r in (_coco_run(name, cuda, order=range(n)[::-1], batch=1, debug=False), _coco_run(name, cuda, order=np.roll(np.arange(n), 1), batch=2, debug=False)):
        for key in ('precision', 'recall', 'scores', 'stats', 'npig', 'rank', 'bits'):
            assert r[key].tobytes() == base[key].tobytes(), key


@pytest.mark.parametrize("name", ('waves', 'capacity', 'sortkeys'))
def test_coco_box_iou_called_directly(cuda, name):
    from scda_amd import native as N
    images = coco_evaluated(name)[0]
    D, G = edges.COCO_CAPS[name]
    args, _ = _coco_batch(images, list(range(len(images))), D, G, cuda)
    xywh = np.zeros((len(images), D, 4))
    for b, im in enumerate(images):
        xywh[b, :len(im['dt_score'])] = im['dt_xywh']
    got = N.coco_box_iou(_dev(xywh, cuda), args[2], args[3], args[7], args[5]).cpu().numpy()
    assert got.shape == (len(images), G, D)
    for b, im in enumerate(images):
        g, d = len(im['gt_cat']), len(im['dt_score'])
        assert got[b, :g, :d].tobytes() == im['iou'].reshape(g, d).tobytes(), (name, b)
        assert not got[b, g:].any() and not got[b, :, d:].any()               # nothing is written past the counts
    assert sum(im['iou'].size for im in images) > 0 and max(float(im['iou'].max()) for im in images if im['iou'].size) > 0.5


# ------------------------------------------------------------------------------------------------ Cityscapes mAP
def _map_batch(images, caps, cuda):
    """all images of a set as the tensors MapEvaluator.add takes; the padding rows hold values that would count if they were read"""
    B, D, G = len(images), caps['D'], caps['G']
    det = np.zeros((B, D, 7), np.float32); dc = np.zeros(B, np.int32); gc = np.zeros(B, np.int32)
    det[:, :, 1:] = (3, 3, 60, 60, 2.0, 1)
    gb = np.tile(np.asarray([3, 3, 60, 60, 1], np.int32), (B, G, 1))
    info = np.stack([im['info'] for im in images])
    for b, im in enumerate(images):
        dc[b], gc[b] = len(im['det']), len(im['gt'])
        det[b, :dc[b]], gb[b, :gc[b]] = im['det'], im['gt']
    args = [_dev(a, cuda) for a in (det, dc, info, gb, gc)]
    kw = {}
    if 'props' in images[0]:
        P, RG = caps['P'], caps['RG']
        pr = np.zeros((B, P, 6), np.float32); pc = np.zeros(B, np.int32); rg = np.zeros((B, RG, 5), np.float32); rc = np.zeros(B, np.int32)
        pr[:, :, 1:5], rg[:, :, :4] = (0, 0, 1023, 511), (0, 0, 1023, 511)
        for b, im in enumerate(images):
            pc[b], rc[b] = len(im['props']), len(im['rgts'])
            pr[b, :pc[b]], rg[b, :rc[b]] = im['props'], im['rgts']
        kw = {'proposals': _dev(pr, cuda), 'proposal_counts': _dev(pc, cuda), 'recall_gts': _dev(rg, cuda), 'recall_gt_counts': _dev(rc, cuda)}
    return args, kw


def _map_default(name, cuda):
    if ('map', name) not in _RUNS:
        from scda_amd.map_eval import MapEvaluator
        images, C, sum_gt, _ = map_evaluated(name)
        caps = edges.MAP_CAPS[name]
        ev = MapEvaluator(C, max_images=len(images), max_dets_per_image=caps['D'], max_gts_per_image=caps['G'], device=cuda,
                          keep_num=caps['keep_num'], sum_gt=sum_gt, debug=True)
        args, kw = _map_batch(images, caps, cuda)
        ev.add(*args, **kw)
        _RUNS['map', name] = _collect(ev, images)
    return _RUNS['map', name]


@pytest.mark.parametrize("name", edges.MAP_SETS)
def test_map_rows_equal_rule_r1(cuda, name):
    got, res = _map_default(name, cuda), map_evaluated(name)[3]
    assert np.array_equal(got['rank'], np.concatenate([e['rank'] for e in res['per_image']]))
    assert np.array_equal(got['kept'], np.concatenate([e['kept'] for e in res['per_image']]).astype(np.int32))
    assert np.array_equal(got['box'], np.concatenate([e['box'] for e in res['per_image']]))
    assert np.array_equal(got['cls'], np.concatenate([e['cls'] for e in res['per_image']]))
    assert got['kept'].sum() == len(map_fixture()[name + '_res'])


@pytest.mark.parametrize("name", edges.MAP_SETS)
def test_map_matching_equals_the_recorded_and_the_statement(cuda, name):
    z, got, res = map_fixture(), _map_default(name, cuda), map_evaluated(name)[3]
    assert np.array_equal(got['tp'], z[name + '_tp']) and np.array_equal(got['tp'], np.concatenate([e['tp'] for e in res['per_image']]))
    assert np.array_equal(got['match'], z[name + '_match']) and np.array_equal(got['match'], np.concatenate([e['match'] for e in res['per_image']]))
    assert np.array_equal(got['claimed'], z[name + '_is_det']) and np.array_equal(got['claimed'], np.concatenate([e['claimed'] for e in res['per_image']]))


@pytest.mark.parametrize("name", edges.MAP_SETS)
def test_map_ap_is_bit_equal_to_the_reference(cuda, name):
    z, got, res = map_fixture(), _map_default(name, cuda), map_evaluated(name)[3]
    C = int(z[name + '_C'])
    for k in ('ap', 'max_recall'):
        want = z[name + '_' + k]
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want, equal_nan=True), (k, got[k], want)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want))
        fin = np.isfinite(want)
        assert got[k][fin].tobytes() == want[fin].tobytes() == res[k][fin].tobytes(), k
    assert np.array_equal(got['mAP'], z[name + '_mAP'], equal_nan=True)
    assert np.array_equal(got['rows'], np.bincount(z[name + '_res'][:, 0], minlength=C)) and np.array_equal(got['sum_gt'], z[name + '_sum_gt'])
    if name == 'recall':
        assert (got['rpn_recalled'], got['rpn_gts']) == (int(z['recall_recalled']), int(z['recall_rpn_gts']))
    else:
        assert got['rpn_gts'] == 0


def test_map_recall_called_directly(cuda):
    """image by image and in one launch, against voc_map_np.recall and compute_recall's recorded answers"""
    from scda_amd import native as N
    z = map_fixture()
    images = map_evaluated('recall')[0]
    _, kw = _map_batch(images, edges.MAP_CAPS['recall'], cuda)
    pr, pc, rg, rc = kw['proposals'], kw['proposal_counts'], kw['recall_gts'], kw['recall_gt_counts']
    want = np.asarray([vnp.recall(im['props'], im['rgts']) for im in images], dtype=np.int32)
    assert np.array_equal(want, z['recall_recalled_each'])
    each = torch.zeros(len(images), 2, dtype=torch.int32, device=cuda)
    for b in range(len(images)):
        N.map_recall(pr[b:b + 1], pc[b:b + 1], rg[b:b + 1], rc[b:b + 1], each[b])
    assert np.array_equal(each.cpu().numpy(), want), (each.cpu().numpy(), want)
    total = torch.zeros(2, dtype=torch.int32, device=cuda)
    N.map_recall(pr, pc, rg, rc, total)
    N.map_recall(pr, pc, rg, rc, total)                                      # the counters add up
    assert total.cpu().numpy().tolist() == (2 * want.sum(0)).tolist()
