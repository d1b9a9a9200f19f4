"""Cityscapes mAP on the MI355X (scda_amd/csrc/map_eval.hip, scda_amd/map_eval.py) against the arrays recorded from the reference's own
utils/cal_mAP.py and compute_recall (tests/golden/voc_map_ref.npz, eval_*.npz) and against the numpy statement of the rules
(tests/voc_map_np.py): rows, matching, ap / max_recall and the recall counters bit for bit, independence of the batching, two runs giving
the same bytes, the capacity contract, and Predictor -> evaluate.map_stats end to end against the host path (infer.rows,
evaluate.detection_rows, the rules in numpy)."""
import numpy as np
import pytest
import torch

import voc_map_np as vnp
from test_voc_map_rules import EVAL_FILES, NUM_CLASSES_EVAL, SETS, eval_case, evaluated, fixture

pytestmark = pytest.mark.gpu

CAPS = {'rules': (136, 72), 'nan': (4, 2), 'random': (100, 32)}              # (detection slots, GT slots) per image
P_CAP, RG_CAP = 64, 32                                                       # proposal and recall ground-truth slots of 'random'
IMAGE_SEEDS = (56, 67, 69, 72)             # synthetic images on which the seeded detector gives no two kept rows of an image one score


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _batch(images, idx, D, G, cuda):
    """the images idx as the tensors MapEvaluator.add takes; the padding rows hold values that would count if they were read"""
    B = len(idx)
    det = np.zeros((B, D, 7), np.float32); dc = np.zeros(B, np.int32); gc = np.zeros(B, np.int32)
    det[:, :, 1:] = (3, 3, 60, 60, 2.0, 1)
    gb = np.tile(np.asarray([3, 3, 60, 60, 1], np.int32), (B, G, 1))
    info = np.stack([images[i]['info'] for i in idx])
    for b, i in enumerate(idx):
        im = images[i]
        dc[b], gc[b] = len(im['det']), len(im['gt'])
        det[b, :dc[b]], gb[b, :gc[b]] = im['det'], im['gt']
    args = [_dev(a, cuda) for a in (det, dc, info, gb, gc)]
    kw = {}
    if 'props' in images[idx[0]]:
        pr = np.zeros((B, P_CAP, 6), np.float32); pc = np.zeros(B, np.int32); rg = np.zeros((B, RG_CAP, 5), np.float32); rc = np.zeros(B, np.int32)
        pr[:, :, 1:5], rg[:, :, :4] = (0, 0, 1023, 511), (0, 0, 1023, 511)
        for b, i in enumerate(idx):
            im = images[i]
            pc[b], rc[b] = len(im['props']), len(im['rgts'])
            pr[b, :pc[b]], rg[b, :rc[b]] = im['props'], im['rgts']
        kw = {'proposals': _dev(pr, cuda), 'proposal_counts': _dev(pc, cuda), 'recall_gts': _dev(rg, cuda), 'recall_gt_counts': _dev(rc, cuda)}
    return args, kw


def _collect(ev, images):
    """the evaluator's state and summary as host arrays, the per-row ones cut to the images' real rows"""
    res = ev.summarize()
    cut = lambda t, key: np.concatenate([t[i, :len(im[key])] for i, im in enumerate(images)])    # noqa: E731
    for k in ('box', 'rank', 'kept', 'tp', 'cls'):
        res[k] = cut(getattr(ev, k).cpu().numpy(), 'det')
    if ev.debug_match is not None:
        res['match'], res['claimed'] = cut(ev.debug_match.cpu().numpy(), 'det'), cut(ev.debug_claimed.cpu().numpy(), 'gt')
    return res


def _run(name, cuda, splits=None, debug=True, ev=None):
    """the set through a MapEvaluator, the images in the fixture's order, cut into batches of the sizes `splits` (default: one batch)"""
    from scda_amd.map_eval import MapEvaluator
    images, C, sum_gt = vnp.load_set(fixture(), name)
    D, G = CAPS[name]
    if ev is None:
        ev = MapEvaluator(C, max_images=len(images), max_dets_per_image=D, max_gts_per_image=G, device=cuda, keep_num=min(100, D),
                          sum_gt=sum_gt, debug=debug)
    splits = [len(images)] if splits is None else splits
    assert sum(splits) == len(images)
    at = 0
    for n in splits:
        args, kw = _batch(images, list(range(at, at + n)), D, G, cuda)
        ev.add(*args, **kw)
        at += n
    return _collect(ev, images), ev


_RUNS = {}


def _default_run(name, cuda):
    if name not in _RUNS:
        _RUNS[name] = _run(name, cuda)[0]
    return _RUNS[name]


def _same_bytes(a, b, keys=('ap', 'max_recall', 'rows', 'sum_gt', 'tp', 'box', 'rank', 'kept')):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and \
        (a['rpn_recalled'], a['rpn_gts']) == (b['rpn_recalled'], b['rpn_gts'])


@pytest.mark.parametrize("name", SETS)
def test_rows_equal_rule_r1(cuda, name):
    got, res = _default_run(name, cuda), evaluated(name)[3]
    assert np.array_equal(got['rank'], np.concatenate([e['rank'] for e in res['per_image']]))
    assert np.array_equal(got['kept'], np.concatenate([e['kept'] for e in res['per_image']]).astype(np.int32))
    assert np.array_equal(got['box'], np.concatenate([e['box'] for e in res['per_image']]))
    assert got['kept'].sum() == len(fixture()[name + '_res'])


@pytest.mark.parametrize("name", SETS)
def test_matching_equals_the_reference(cuda, name):
    z, got, res = fixture(), _default_run(name, cuda), evaluated(name)[3]
    assert np.array_equal(got['tp'], z[name + '_tp']) and np.array_equal(got['tp'], np.concatenate([e['tp'] for e in res['per_image']]))
    assert np.array_equal(got['match'], z[name + '_match'])
    assert np.array_equal(got['claimed'], z[name + '_is_det'])


@pytest.mark.parametrize("name", SETS)
def test_ap_is_bit_equal_to_the_reference(cuda, name):
    z, got = fixture(), _default_run(name, cuda)
    C = int(z[name + '_C'])
    for k in ('ap', 'max_recall'):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], z[name + '_' + k], equal_nan=True), (k, got[k], z[name + '_' + k])
        assert np.array_equal(np.isnan(got[k]), np.isnan(z[name + '_' + k]))
    assert np.array_equal(got['mAP'], z[name + '_mAP'], equal_nan=True)
    assert np.array_equal(got['rows'], np.bincount(z[name + '_res'][:, 0], minlength=C)) and np.array_equal(got['sum_gt'], z[name + '_sum_gt'])
    if name == 'nan':
        assert np.isnan(got['ap'][2]) and np.isnan(got['max_recall'][2])
    if name == 'random':
        assert (got['rpn_recalled'], got['rpn_gts']) == (int(z['random_recalled']), int(z['random_rpn_gts']))
        assert got['rpn_recall'] == int(z['random_recalled']) / int(z['random_rpn_gts'])


def test_counted_ground_truths_stand_in_for_the_meta_counts(cuda):
    """sum_gt=None: the ground truths of the images added ('random' adds every meta image, so nothing changes)"""
    from scda_amd.map_eval import MapEvaluator
    images, C, sum_gt = vnp.load_set(fixture(), 'random')
    D, G = CAPS['random']
    ev = MapEvaluator(C, max_images=len(images), max_dets_per_image=D, max_gts_per_image=G, device=cuda)
    args, _ = _batch(images, list(range(len(images))), D, G, cuda)
    ev.add(*args)
    got = ev.summarize()
    assert np.array_equal(got['sum_gt'], sum_gt) and got['ap'].tobytes() == fixture()['random_ap'].tobytes()
    assert got['rpn_gts'] == 0 and np.isnan(got['rpn_recall'])


@pytest.mark.parametrize("file", EVAL_FILES)
@pytest.mark.parametrize("tag", ["", "3"])
def test_eval_path_rows_give_the_recorded_ap(cuda, file, tag):
    from scda_amd.map_eval import MapEvaluator
    images, gt, ap, max_recall, m = eval_case(file, tag)
    G = max(len(im['gt']) for im in images)
    ev = MapEvaluator(NUM_CLASSES_EVAL, max_images=len(images), max_dets_per_image=100, max_gts_per_image=G, device=cuda, sum_gt=gt['num'])
    args, _ = _batch(images, list(range(len(images))), 100, G, cuda)
    ev.add(*args)
    got = ev.summarize()
    assert np.array_equal(got['ap'], ap, equal_nan=True) and np.array_equal(got['max_recall'], max_recall, equal_nan=True)
    assert np.array_equal(got['mAP'], m, equal_nan=True)


def test_batching_does_not_change_a_byte(cuda):
    whole = _default_run('random', cuda)
    n = len(fixture()['random_names'])
    ragged = [3, 1, 7, 2, 11, 1, 5, 10]
    assert sum(ragged) == n
    for splits in ([1] * n, ragged):
        assert _same_bytes(_run('random', cuda, splits)[0], whole), splits


def test_two_runs_give_the_same_bytes(cuda):
    first, ev = _run('random', cuda)
    ev.reset()
    again, _ = _run('random', cuda, ev=ev)
    assert _same_bytes(first, again) and _same_bytes(first, _default_run('random', cuda))
    assert first['match'].tobytes() == again['match'].tobytes() and first['claimed'].tobytes() == again['claimed'].tobytes()


def test_capacity_contract(cuda):
    from scda_amd import native as N
    from scda_amd.map_eval import MapEvaluator
    images, C, sum_gt = vnp.load_set(fixture(), 'nan')
    with pytest.raises(ValueError):
        MapEvaluator(C, max_images=2, max_dets_per_image=4, max_gts_per_image=2, device=cuda, keep_num=5)
    with pytest.raises(ValueError):
        MapEvaluator(C, max_images=2, max_dets_per_image=1025, max_gts_per_image=2, device=cuda)
    ev = MapEvaluator(C, max_images=1, max_dets_per_image=4, max_gts_per_image=2, device=cuda, keep_num=4)
    args, _ = _batch(images, [0, 1], 4, 2, cuda)
    with pytest.raises(ValueError):
        ev.add(*args)                                                        # too many images
    args, _ = _batch(images, [0], 4, 2, cuda)
    with pytest.raises(ValueError):
        ev.add(args[0][:, :, :6].contiguous(), *args[1:])                    # a wrong detection width
    with pytest.raises(ValueError):
        ev.add(args[0][:, :3].contiguous(), *args[1:])                       # not the evaluator's slot count
    with pytest.raises(ValueError):
        ev.add(*args[:3], args[3][:, :1].contiguous(), args[4])              # not the evaluator's ground-truth capacity
    with pytest.raises(ValueError):
        ev.accumulate()                                                      # nothing was added
    assert ev.n_images == 0 and int(ev.gt_num.sum()) == 0 and int(ev.tp.sum()) == 0
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=cuda)         # noqa: E731
    with pytest.raises(N.ScdaNativeError):                                   # the C entry point refuses keep_num > D itself
        N.map_rows(args[0], args[1], args[2], -1, C, 5, i32(1, 4, 4), torch.zeros(1, 4, device=cuda), i32(1, 4), i32(1, 4), i32(1, 4), i32(1, 4))
    assert N.map_accumulate_workspace_bytes(1, 1025) == 0 and N.map_accumulate_workspace_bytes(500, 100) > 0
    ev.add(*args)
    assert ev.n_images == 1 and ev.summarize()['rows'].tolist() == [0, 1, 1]


def test_predictor_to_map_stats_equals_the_host_path(cuda):
    """one Predictor pass feeds map_stats; the same output tensors go through infer.rows, evaluate.detection_rows and the rules in numpy"""
    from test_eval_path import si
    from test_host_functions import CFG
    from test_infer_gpu import _detector
    from scda_amd import evaluate, infer
    from scda_amd.map_eval import MapEvaluator
    H, W, G, C, scale = 256, 512, 8, int(CFG['shared']['num_classes']), 0.5
    det = _detector(cuda)
    imgs = torch.cat([si.synth_images(s, H, W)[0] for s in IMAGE_SEEDS], 0)
    info = torch.tensor([[H, W, scale]] * 4)
    rgts = torch.stack([si.synth_gts(G, s, H, W).reshape(G, 5) for s in (61, 62, 63, 64)]).float()
    names = ["leftImg8bit/val/city/img%d_leftImg8bit.png" % b for b in range(4)]
    pred = infer.Predictor(det, CFG)
    # the ground truth is cut from a first pass: every third detection's box in the original image's coordinates, so some rows match
    d0, dc0 = (t.cpu().numpy() for t in pred(imgs.to(cuda), info)[2:4])
    gt = {'num': np.zeros(C, dtype=np.int64)}
    for b in range(3):                                                       # the fourth image is absent from the meta
        rows = vnp.image_rows(d0[b, :dc0[b]], info[b].numpy(), C)
        pick = [d for d in rows['order'][::3]][:16]
        gt["img%d_leftImg8bit" % b] = np.concatenate([rows['box'][pick], rows['cls'][pick, None]], 1).astype(np.int32)
        gt['num'] += np.bincount(rows['cls'][pick], minlength=C)
    ev = MapEvaluator(C, max_images=4, max_dets_per_image=pred.top_n, max_gts_per_image=16, device=cuda, sum_gt=gt['num'])
    got = evaluate.map_stats([(imgs, info, rgts, names)], pred, ev, gt)
    # ---- the host path over the SAME output tensors
    props, dets = infer.rows(*pred._out[:4])
    text, rc, ng = [], 0, 0
    for b in range(4):
        mine = dets[dets[:, 0] == b]
        kept = np.sort(mine[:, 5])[::-1][:100]
        assert len(np.unique(kept)) == len(kept), "two kept rows of image %d share a score: choose another seed" % b
        text += evaluate.detection_rows("img%d_leftImg8bit" % b, mine, rgts[b].numpy(), info[b].numpy(), C, info[b, -1].numpy())
        r, g = vnp.recall(props[props[:, 0] == b], rgts[b].numpy())
        rc, ng = rc + r, ng + g
    images = vnp.parse_text_rows(''.join(text))
    for im in images:
        im['info'], im['gt'] = np.asarray([4096, 4096, 1.0], np.float32), gt.get(im['name'], np.zeros((0, 5), np.int32))
    want = vnp.evaluate(images, C, sum_gt=gt['num'])
    assert np.array_equal(got['ap'], want['ap'], equal_nan=True) and np.array_equal(got['max_recall'], want['max_recall'], equal_nan=True)
    assert np.array_equal(got['rows'], want['rows']) and got['rows'].sum() > 0 and int(ev.tp.sum()) > 0
    assert (got['rpn_recalled'], got['rpn_gts']) == (rc, ng) and ng == 4 * G
