"""Merging sharded device evaluators on the MI355X (scda_amd/csrc/eval_merge.hip, StreamingEvaluator.absorb / merge): per-rank
MapEvaluators over DistributedSampler shards, absorbed in merge_order, against what the reference's own cal_mAP gave for the
concatenated rank files (tests/golden/sharded_map_ref.npz) -- ap, max_recall and rows byte for byte, tp flag for flag --; the device
flags; CocoEvaluator shards against one evaluator over all images; two ranks over gloo on one GPU and a one-rank RCCL group."""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sharded_map_np as snp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

MAP_CAPS = {'random': (100, 32), 'hand': (4, 2), 'zero': (4, 2)}             # (detection slots, GT slots) per image
JOIN_SECONDS = 150


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _map_evaluator(case, cuda, max_images, **kw):
    from scda_amd.map_eval import MapEvaluator
    images, C, ids, sum_gt, shards = snp.load_case(case)
    D, G = MAP_CAPS[snp.CASES[case][0]]
    return MapEvaluator(C, max_images=max_images, max_dets_per_image=D, max_gts_per_image=G, device=cuda, keep_num=min(100, D),
                        sum_gt=sum_gt, **kw)


def _add(ev, case, idx, cuda, with_ids=True, ids=None):
    from test_voc_map_gpu import _batch
    images, C, case_ids, sum_gt, shards = snp.load_case(case)
    if not idx:
        return ev
    args, kw = _batch(images, list(idx), ev.D, ev.G, cuda)
    if with_ids:
        kw['image_ids'] = _dev(np.asarray(case_ids if ids is None else ids, np.int32)[list(idx)], cuda)
    ev.add(*args, **kw)
    return ev


def _shard_evaluators(case, cuda, max_images):
    shards = snp.load_case(case)[4]
    return [_add(_map_evaluator(case, cuda, max_images), case, s, cuda) for s in shards]


def _tp_of(ev, case, merged):
    images = snp.load_case(case)[0]
    tp = ev.tp.cpu().numpy()
    return np.concatenate([tp[p, :len(images[i]['det'])] for p, i in enumerate(merged)] + [np.zeros(0, np.int32)])


def _same_summary(a, b, keys=('ap', 'max_recall', 'rows', 'sum_gt')):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and \
        (a['rpn_recalled'], a['rpn_gts']) == (b['rpn_recalled'], b['rpn_gts'])


# ------------------------------------------------------------------------------------------------ in-process map merge
@pytest.mark.parametrize("case", list(snp.CASES))
def test_absorbed_shards_equal_the_reference_over_the_concatenated_rank_files(cuda, case):
    from scda_amd.map_eval import merge_order
    z = snp.fixture()
    shards = snp.load_case(case)[4]
    W = len(shards)
    merged = snp.merged_images(shards, snp.merge_order(W))
    evs = _shard_evaluators(case, cuda, len(merged))
    ev = _map_evaluator(case, cuda, len(merged)).absorb(evs, order=merge_order(W))
    got = ev.summarize()
    assert ev.n_images == len(merged)
    for k in ('ap', 'max_recall'):
        assert got[k].dtype == np.float64 and got[k].tobytes() == z[case + '_' + k].tobytes(), (k, got[k], z[case + '_' + k])
    assert got['rows'].tobytes() == z[case + '_rows'].astype(np.int32).tobytes()
    assert np.array_equal(_tp_of(ev, case, merged), z[case + '_tp'])
    flags = ev.merge_flags.cpu().numpy()
    assert flags[:3].tolist() == [0, 0, int(z[case + '_duplicates'])]
    first = ev._merge_first.cpu().numpy()[:len(merged)]
    ids = snp.load_case(case)[2]
    assert np.array_equal(first, snp.first_positions([ids[i] for i in merged]))
    parts = [e.summarize() if e.n_images else None for e in evs]             # the counters are the sums over the shards
    assert got['rpn_gts'] == sum(p['rpn_gts'] for p in parts if p) and got['rpn_recalled'] == sum(p['rpn_recalled'] for p in parts if p)
    assert np.array_equal(ev.gt_num.cpu().numpy(), sum(e.gt_num.cpu().numpy() for e in evs))


def test_the_order_of_the_shards_is_honoured(cuda):
    z = snp.fixture()
    evs = _shard_evaluators('w11', cuda, 11)
    numeric = _map_evaluator('w11', cuda, 11).absorb(evs, order=list(range(11))).summarize()
    assert numeric['ap'].tobytes() != z['w11_ap'].tobytes() and numeric['ap'].tobytes() == z['w11_ap_numeric'].tobytes()
    default = _map_evaluator('w11', cuda, 11).absorb(evs).summarize()        # order=None: as given
    assert default['ap'].tobytes() == numeric['ap'].tobytes()
    with pytest.raises(ValueError):
        _map_evaluator('w11', cuda, 11).absorb(evs, order=[0] * 11)


def test_one_absorbed_shard_equals_todays_single_evaluator(cuda):
    shard = snp.load_case('w2')[4][0]
    single = _add(_map_evaluator('w2', cuda, 40), 'w2', shard, cuda, with_ids=False)         # as ever: no ids
    want = single.summarize()
    ev = _map_evaluator('w2', cuda, 40).absorb([_add(_map_evaluator('w2', cuda, 40), 'w2', shard, cuda)])
    got = ev.summarize()
    assert _same_summary(got, want) and got['mAP'].tobytes() == want['mAP'].tobytes()
    n = len(shard)
    for k in ('box', 'score', 'cls', 'rank', 'kept', 'tp'):
        assert torch.equal(getattr(ev, k)[:n], getattr(single, k)[:n]), k
    # absorbing in two steps appends: the second shard behind the first
    evs = _shard_evaluators('w2', cuda, 40)
    both = _map_evaluator('w2', cuda, 40).absorb(evs).summarize()
    steps = _map_evaluator('w2', cuda, 40).absorb(evs[:1]).absorb(evs[1:]).summarize()
    assert _same_summary(both, steps) and both['ap'].tobytes() == snp.fixture()['w2_ap'].tobytes()


# ------------------------------------------------------------------------------------------------ flags
def test_a_duplicate_with_a_different_score_raises(cuda):
    from test_voc_map_gpu import _batch
    images, C, ids, sum_gt, shards = snp.load_case('zero')
    i = next(k for k in range(5) if len(images[k]['det']) >= 2)
    a = _add(_map_evaluator('zero', cuda, 4), 'zero', [i], cuda)
    b = _map_evaluator('zero', cuda, 4)
    args, kw = _batch(images, [i], b.D, b.G, cuda)
    args[0][0, 1, 5] += 0.125                                                # one row's score
    b.add(*args, image_ids=_dev(np.asarray([ids[i]], np.int32), cuda), **kw)
    ev = _map_evaluator('zero', cuda, 4).absorb([a, b])
    with pytest.raises(ValueError, match="duplicate image with different detections: not covered"):
        ev.summarize()
    same = _map_evaluator('zero', cuda, 4).absorb([a, _add(_map_evaluator('zero', cuda, 4), 'zero', [i], cuda)])
    assert same.summarize()['rows'].sum() == 2 * len(images[i]['det']) and int(same.tp[1].sum()) == 0 and int(same.tp[0].sum()) > 0


def test_a_merged_total_above_max_images_raises(cuda):
    evs = [_add(_map_evaluator('zero', cuda, 3), 'zero', idx, cuda) for idx in ([0, 1], [2, 3])]
    ev = _map_evaluator('zero', cuda, 3)
    with pytest.raises(ValueError, match="max_images"):
        ev.absorb(evs)
        ev.summarize()
    assert ev.n_images == 0


def test_device_counts_fill_every_slot_and_raise_the_flag(cuda):
    """the placement as merge() uses it over device collectives: the counts live on the device only"""
    from scda_amd import native as N
    W, cap, D, I = 3, 4, 5, 7
    src = torch.arange(W * cap * D, dtype=torch.int32, device=cuda).reshape(W, cap, D) + 100
    flags = torch.zeros(4, dtype=torch.int32, device=cuda)
    dst = torch.full((I, D), -7, dtype=torch.int32, device=cuda)
    N.eval_place_rows(src, [2, 0, 1], _dev(np.asarray([2, 0, 1], np.int32), cuda), 1, dst, flags, fill="slot")
    want = torch.cat([torch.full((1, D), -7, dtype=torch.int32, device=cuda), src[2, :1], src[0, :2],
                      torch.arange(D, dtype=torch.int32, device=cuda).repeat(3, 1)])
    assert torch.equal(dst, want) and flags.tolist() == [0, 0, 0, 4]
    ids = torch.full((I,), 5, dtype=torch.int32, device=cuda)
    N.eval_place_rows(src[:, :, :1].contiguous().reshape(W, cap), [0, 1, 2], _dev(np.asarray([9, 4, 4], np.int32), cuda), 0, ids, flags,
                      fill="minus_one")                                      # 9 is clamped to the capacity 4; 12 images > 7 slots
    assert ids.tolist() == [100, 105, 110, 115, 120, 125, 130] and flags.tolist() == [1, 0, 0, 7]
    f64 = torch.arange(W * cap * 2, dtype=torch.float64, device=cuda).reshape(W, cap, 2)
    out = torch.zeros(I, 2, dtype=torch.float64, device=cuda)
    N.eval_place_rows(f64, [1, 0, 2], [1, 2, 0], 0, out, flags)              # host counts, 8-byte rows: only the total's slots
    assert torch.equal(out[:3], torch.stack([f64[1, 0], f64[1, 1], f64[0, 0]])) and float(out[3:].abs().sum()) == 0
    with pytest.raises(N.ScdaNativeError):
        N.eval_place_rows(f64, [0, 1, 2], [4, 4, 4], 0, out, flags)          # refused before anything is launched
    with pytest.raises(N.ScdaNativeError):
        N.eval_place_rows(f64, [0, 1, 1], [1, 1, 1], 0, out, flags)


def test_ids_of_minus_one_are_never_duplicates(cuda):
    images, C, ids, sum_gt, shards = snp.load_case('zero')
    none = np.full(5, -1, np.int32)
    i = next(k for k in range(5) if len(images[k]['det']) >= 2)
    evs = [_add(_map_evaluator('zero', cuda, 4), 'zero', [i], cuda, ids=none) for _ in range(3)]
    ev = _map_evaluator('zero', cuda, 4).absorb(evs)
    ev.summarize()
    assert ev.merge_flags.tolist()[:3] == [0, 0, 0] and int(ev.tp[1].sum()) == int(ev.tp[0].sum()) > 0
    assert ev._merge_first[:3].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError, match="image_ids"):                       # an image added without any id cannot be merged
        _map_evaluator('zero', cuda, 4).absorb([_add(_map_evaluator('zero', cuda, 4), 'zero', [i], cuda, with_ids=False)])


def test_add_after_merge_raises_until_reset(cuda):
    ev = _add(_map_evaluator('zero', cuda, 4), 'zero', [1, 2], cuda)
    before = ev.summarize()
    ev.merge()                                                               # no process group: a merge of one rank
    assert _same_summary(ev.summarize(), before) and ev.n_images == 2
    with pytest.raises(ValueError, match="reset"):
        _add(ev, 'zero', [3], cuda)
    ev.reset()
    assert _same_summary(_add(ev, 'zero', [1, 2], cuda).summarize(), before)


# ------------------------------------------------------------------------------------------------ COCO
def _coco_evaluator(name, cuda, max_images=None, spare=0):
    """-> (an evaluator of max_images (default: the set's images) + spare image slots, the set's images)"""
    import coco_eval_np as cnp
    from test_coco_eval_gpu import CAPS
    from test_coco_eval_rules import fixture
    from scda_amd.coco_eval import CocoEvaluator
    images, K, params = cnp.load_set(fixture(), name)
    D, G = CAPS[name]
    max_images = (len(images) if max_images is None else max_images) + spare
    return CocoEvaluator(K, 'bbox', max_images=max_images, max_dets_per_image=D, max_gts_per_image=G, device=cuda,
                         params={'area_rng': params['area_rng']}), images


def _coco_add(ev, images, idx, cuda):
    from test_coco_eval_gpu import _batch
    if idx:
        ev.add(*_batch(images, list(idx), ev.D, ev.G, cuda)[0])
    return ev


def _coco_result(ev):
    res = {k: v.cpu().numpy().copy() for k, v in ev.accumulate().items()}
    res['stats'] = ev.summarize()
    return res


@pytest.mark.parametrize("name", ('rules', 'random_bbox'))
def test_coco_shards_equal_one_evaluator_over_all_images(cuda, name):
    ev, images = _coco_evaluator(name, cuda)
    n = len(images)
    whole = _coco_result(_coco_add(ev, images, range(n), cuda))
    for W in (2, 3):
        shards = [_coco_add(_coco_evaluator(name, cuda, n)[0], images, range(r, n, W), cuda) for r in range(W)]
        merged = _coco_evaluator(name, cuda, n)[0].absorb(shards, order=snp.merge_order(W))
        got = _coco_result(merged)
        for k in ('precision', 'recall', 'scores', 'stats'):
            assert got[k].tobytes() == whole[k].tobytes(), (W, k)
        assert torch.equal(merged.npig, ev.npig) and merged.merge_flags.tolist()[:3] == [0, 0, 0]


def test_a_repeated_coco_image_id_raises(cuda):
    ev, images = _coco_evaluator('random_bbox', cuda, 8)
    shards = [_coco_add(_coco_evaluator('random_bbox', cuda, 8)[0], images, idx, cuda) for idx in ([0, 1, 2], [3, 0])]
    ev.absorb(shards)
    with pytest.raises(ValueError, match="duplicate image id"):
        ev.summarize()
    assert ev.merge_flags.tolist()[1:3] == [1, 1]


# ------------------------------------------------------------------------------------------------ process groups
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _join(ctx):
    """the workers under a deadline; a hung collective ends the test, it is not tried again"""
    deadline = time.monotonic() + JOIN_SECONDS
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.terminate()
            pytest.fail("the workers did not finish within %d s" % JOIN_SECONDS)


class _Replay:
    """stands in for an infer.Predictor: the image tensor carries the image's index, the results are the fixture's"""

    def __init__(self, images, cuda):
        self.images, self.cuda = images, cuda

    def __call__(self, img, info):
        from test_voc_map_gpu import _batch
        args, kw = _batch(self.images, [int(v) for v in img[:, 0, 0, 0].cpu()], 100, 32, self.cuda)
        self.image_info = args[2]
        return kw['proposals'], kw['proposal_counts'], args[0], args[1]


def _gloo_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    cuda = torch.device("cuda", 0)
    shards = snp.load_case('w2')[4]
    ev = _add(_map_evaluator('w2', cuda, 40), 'w2', shards[rank], cuda)
    own = ev.summarize()
    ev.merge(shard_capacity=20)
    got = ev.summarize()
    # the same through evaluate.map_stats(distributed=True): a loader over this rank's shard, the fixture's detections replayed
    from scda_amd import evaluate
    images, C, ids, sum_gt, _ = snp.load_case('w2')
    gt = {'num': sum_gt}
    gt.update({im['name']: im['gt'] for im in images})
    loader = [(torch.tensor(part, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, 3, 1, 1), torch.from_numpy(np.stack([images[i]['info'] for i in part])),
               torch.zeros(len(part), 1, 5), ["val/city/%s.png" % images[i]['name'] for i in part])
              for part in (shards[rank][:7], shards[rank][7:])]
    replay = _Replay(images, cuda)
    local = evaluate.map_stats(loader, replay, _map_evaluator('w2', cuda, 40), gt)
    stats = evaluate.map_stats(loader, replay, _map_evaluator('w2', cuda, 40), gt, distributed=True)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), ap=got['ap'], max_recall=got['max_recall'], rows=got['rows'], own_ap=own['ap'],
             n_images=ev.n_images, flags=ev.merge_flags.cpu().numpy(), rpn=np.asarray([got['rpn_recalled'], got['rpn_gts']]),
             stats_ap=stats['ap'], stats_max_recall=stats['max_recall'], local_ap=local['ap'])
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_over_gloo_merge_to_the_reference(cuda, tmp_path):
    z = snp.fixture()
    ctx = mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    _join(ctx)
    res = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(2)]
    for r in res:
        assert r['ap'].tobytes() == z['w2_ap'].tobytes() and r['max_recall'].tobytes() == z['w2_max_recall'].tobytes()
        assert r['rows'].tobytes() == z['w2_rows'].astype(np.int32).tobytes() and int(r['n_images']) == 40
        assert r['flags'][:3].tolist() == [0, 0, 0] and r['own_ap'].tobytes() != r['ap'].tobytes()
        assert r['stats_ap'].tobytes() == z['w2_ap'].tobytes() and r['stats_max_recall'].tobytes() == z['w2_max_recall'].tobytes()
        assert r['local_ap'].tobytes() == r['own_ap'].tobytes()              # distributed=False: this rank's own result, as ever
    assert res[0]['rpn'].tolist() == res[1]['rpn'].tolist() and res[0]['rpn'][1] > 0


def _rccl_worker(rank, port, out_dir):
    """ONE rank, backend 'nccl' (= RCCL): the device-collective path of merge(), the counts on the device only"""
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("SLURM_PROCID", None)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    cuda = torch.device("cuda", 0)
    torch.cuda.set_device(cuda)
    dist.init_process_group(backend="nccl", rank=0, world_size=1)
    assert dist.get_backend() == "nccl"
    ev = _add(_map_evaluator('w3', cuda, 48), 'w3', range(40), cuda)         # 8 slots more than images: they are filled as empty rows
    plain = ev.summarize()
    ev.merge()
    got = ev.summarize()
    cev, images = _coco_evaluator('random_bbox', cuda, spare=3)              # three slots more than images
    n = len(images)
    cplain = _coco_result(_coco_add(cev, images, range(n), cuda))
    cev.merge()
    cgot = _coco_result(cev)
    np.savez(os.path.join(out_dir, "rccl.npz"), ap=got['ap'], plain_ap=plain['ap'], max_recall=got['max_recall'],
             plain_max_recall=plain['max_recall'], rows=got['rows'], plain_rows=plain['rows'], n_images=ev.n_images,
             flags=ev.merge_flags.cpu().numpy(), rpn=np.asarray([got['rpn_gts'], plain['rpn_gts']]),
             coco=np.stack([cgot['stats'], cplain['stats']]), coco_precision=cgot['precision'], coco_plain_precision=cplain['precision'],
             coco_flags=cev.merge_flags.cpu().numpy(), coco_n=np.asarray([n, cev.n_images]))
    dist.barrier()
    dist.destroy_process_group()


def test_one_rank_rccl_group_leaves_the_summary_unchanged(cuda, tmp_path):
    ctx = mp.spawn(_rccl_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=False)
    _join(ctx)
    r = np.load(str(tmp_path / "rccl.npz"))
    for k in ('ap', 'max_recall', 'rows'):
        assert r[k].tobytes() == r['plain_' + k].tobytes(), k
    assert r['ap'][1:].min() > 0 and int(r['n_images']) == 48 and r['flags'].tolist() == [0, 0, 0, 40]
    assert r['rpn'][0] == r['rpn'][1] > 0
    assert r['coco'][0].tobytes() == r['coco'][1].tobytes() and r['coco_precision'].tobytes() == r['coco_plain_precision'].tobytes()
    assert r['coco_flags'].tolist() == [0, 0, 0, int(r['coco_n'][0])] and r['coco_n'][1] == r['coco_n'][0] + 3
