"""The merge of sharded evaluators on the host (no GPU): merge_order, the numpy statement of the rules M1..M4 (tests/sharded_map_np.py)
against what the reference's own cal_mAP gave for the concatenated rank files (tests/golden/sharded_map_ref.npz), the fixture's own
preconditions, and the defaults of the new arguments."""
import inspect

import numpy as np
import pytest

import sharded_map_np as snp


def test_merge_order_is_the_order_of_the_rank_strings():
    from scda_amd import eval_base, map_eval
    assert map_eval.merge_order(11) == [0, 1, 10, 2, 3, 4, 5, 6, 7, 8, 9]
    assert map_eval.merge_order(1) == [0] and map_eval.merge_order(10) == list(range(10))
    assert map_eval.merge_order(21)[:13] == [0, 1, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 2]
    for world in range(1, 130):
        order = map_eval.merge_order(world)
        assert order == snp.merge_order(world) == eval_base.merge_order(world) and sorted(order) == list(range(world))
        assert [str(r) for r in order] == sorted(str(r) for r in range(world))


def test_new_arguments_default_to_the_present_behaviour():
    from scda_amd import evaluate
    from scda_amd.coco_eval import CocoEvaluator
    from scda_amd.map_eval import MapEvaluator
    assert inspect.signature(MapEvaluator.add).parameters['image_ids'].default is None
    for f in (evaluate.map_stats, evaluate.coco_stats):
        assert inspect.signature(f).parameters['distributed'].default is False
    for cls in (MapEvaluator, CocoEvaluator):
        assert callable(cls.absorb) and callable(cls.merge) and 'image_ids' in [a for a, _ in cls.MERGE_ROWS]
        assert inspect.signature(cls.absorb).parameters['order'].default is None
        assert inspect.signature(cls.merge).parameters['group'].default is None
    assert CocoEvaluator.MERGE_RAISES_ON_DUPLICATE and not MapEvaluator.MERGE_RAISES_ON_DUPLICATE


def test_first_positions():
    assert snp.first_positions([3, -1, 3, 5, -1, 3, 5, 0]).tolist() == [-1, -1, 0, -1, -1, 0, 3, -1]
    assert snp.first_positions([]).tolist() == []


@pytest.mark.parametrize("case", list(snp.CASES))
def test_the_fixture_holds_the_samplers_shards(case):
    _, n, world = snp.CASES[case]
    images, C, ids, sum_gt, shards = snp.load_case(case)
    assert shards == snp.shard_indices(n, world) and len(images) == n and sorted(ids.tolist()) == list(range(n))
    merged = snp.merged_images(shards, snp.merge_order(world))
    assert len(merged) == -(-n // world) * world and int(snp.fixture()[case + '_duplicates']) == len(merged) - n
    assert (case in snp.PADDED) == (len(merged) > n)


@pytest.mark.parametrize("case", list(snp.CASES))
def test_restatement_equals_the_reference(case):
    z = snp.fixture()
    images, C, ids, sum_gt, shards = snp.load_case(case)
    merged = snp.merged_images(shards, snp.merge_order(len(shards)))
    got = snp.evaluate_merged(images, merged, ids, C, sum_gt)
    for k in ('ap', 'max_recall'):
        assert got[k].dtype == np.float64 and got[k].tobytes() == z[case + '_' + k].tobytes(), (k, got[k], z[case + '_' + k])
    assert np.array_equal(got['rows'], z[case + '_rows']) and np.array_equal(got['tp'], z[case + '_tp'])
    assert got['duplicates'] == int(z[case + '_duplicates'])
    if case in snp.PADDED:                     # the rule matters: the ranks' own tp would give another ap
        local = snp.evaluate_merged(images, merged, ids, C, sum_gt, duplicates='local')
        assert local['ap'].tobytes() != z[case + '_ap'].tobytes() and local['tp'].sum() > got['tp'].sum()


def test_the_rank_order_shows_in_the_w11_case():
    z = snp.fixture()
    images, C, ids, sum_gt, shards = snp.load_case('w11')
    numeric = snp.evaluate_merged(images, snp.merged_images(shards, list(range(11))), ids, C, sum_gt)
    assert numeric['ap'].tobytes() == z['w11_ap_numeric'].tobytes() != z['w11_ap'].tobytes()
    assert all(len(s) == 1 for s in shards)                                  # 7 images, 11 ranks: four shards exist by the padding only


def test_structural_cases():
    z = snp.fixture()
    for case in ('h255', 'h256', 'h257', 'h258'):
        assert int(z[case + '_shard_counts'].sum()) == int(case[1:])
    images, C, ids, sum_gt, shards = snp.load_case('h258')
    merged = snp.merged_images(shards, snp.merge_order(3))
    place = sorted(range(len(merged)), key=lambda p: (ids[merged[p]], p))      # the stable sort by id of rule M3
    assert merged[place[255]] == merged[place[256]]                           # the copy is the first position of the second round
    images, C, ids, sum_gt, shards = snp.load_case('zero')
    assert len(images[shards[0][0]]['det']) == 0
    images, C, ids, sum_gt, shards = snp.load_case('few')
    assert max(sum(s.count(i) for s in shards) for i in range(3)) >= 3


def test_fixture_holds_data_only():
    for k, v in snp.fixture().items():
        assert v.dtype.kind in 'iufU', (k, v.dtype)
        if v.dtype.kind == 'U':
            assert k.endswith('_names') and all(len(s) <= 8 for s in v.tolist())
