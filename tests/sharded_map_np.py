"""The merge rules M1..M4 of include/scda_ops.h restated in numpy over the rules R1..R3 of tests/voc_map_np.py: what the reference
computes from `cat results.txt.rank*` when every rank wrote the rows of its DistributedSampler shard.  Used by the tests of
StreamingEvaluator.absorb / merge and by tests/golden/make_golden_sharded_map.py, which asserts it against the reference's own cal_mAP.
Also the layout of the fixture tests/golden/sharded_map_ref.npz."""
import os

import numpy as np

import voc_map_np as vnp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# case -> (image pool, images taken from its start, ranks); 'random' is the pool of tests/golden/voc_map_ref.npz
CASES = {'w2': ('random', 40, 2), 'w3': ('random', 40, 3), 'w8': ('random', 40, 8), 'w11': ('random', 7, 11), 'few': ('hand', 3, 8),
         'h255': ('hand', 254, 3), 'h256': ('hand', 255, 2), 'h257': ('hand', 257, 1), 'h258': ('hand', 257, 3), 'zero': ('zero', 5, 4)}
PADDED = [c for c, (_, n, w) in CASES.items() if n % w]


def merge_order(world):
    """the order of `cat results.txt.rank*`: the decimal rank strings, sorted"""
    return [int(s) for s in sorted(str(r) for r in range(world))]


def shard_indices(n, world):
    """the index list of every rank: torch's DistributedSampler over range(n), shuffled, epoch 0 (it pads by repeating from the start)"""
    from torch.utils.data import DistributedSampler
    return [list(DistributedSampler(range(n), num_replicas=world, rank=r, shuffle=True)) for r in range(world)]


def merged_images(shards, order):
    """M1: the image indices in merged order"""
    return [i for r in order for i in shards[r]]


def first_positions(ids):
    """M3: per merged position the first position of its id when the id >= 0 occurred earlier, else -1"""
    seen, first = {}, []
    for p, i in enumerate(ids):
        i = int(i)
        first.append(seen[i] if i >= 0 and i in seen else -1)
        if i >= 0:
            seen.setdefault(i, p)
    return np.asarray(first, dtype=np.int32)


def evaluate_merged(images, merged, ids, num_classes, sum_gt, keep_num=100, duplicates='false_positive'):
    """R1, R2 per image, M3 + M4 over the merged list, R3 over it.  images: vnp's dicts; merged: image indices in merged order; ids:
    per image its identity (-1: none).  duplicates: 'false_positive' (M4: a later copy's rows stay and get tp = 0) or 'local' (every
    copy keeps the tp its rank computed -- what a merge without M4 would give).
    -> {'ap', 'max_recall', 'rows', 'tp': uint8, flat over the merged images' live rows, 'first', 'duplicates'}"""
    cache = {}
    for i in set(merged):
        rows = vnp.image_rows(images[i]['det'], images[i]['info'], num_classes, keep_num)
        cache[i] = (rows, vnp.match_image(rows, images[i]['gt'], num_classes)[0])
    first = first_positions([ids[i] for i in merged])
    per = []
    for p, i in enumerate(merged):
        rows, tp = cache[i]
        per.append((rows, np.zeros_like(tp) if first[p] >= 0 and duplicates == 'false_positive' else tp))
    ap, max_recall, nrows = vnp.accumulate(per, num_classes, sum_gt)
    return {'ap': ap, 'max_recall': max_recall, 'rows': nrows, 'first': first, 'duplicates': int((first >= 0).sum()),
            'tp': np.concatenate([tp for _, tp in per] + [np.zeros(0, np.int32)]).astype(np.uint8)}


# ---- the fixture's layout: the pools 'hand' and 'zero' as voc_map_np.load_set reads them; per case c: c_ids i32 [n] (the position in
# the meta, which may hold images that are never added), c_sum_gt (the meta's counts), c_shards i32 (the ranks' index lists, flat) with
# c_shard_counts [W]; recorded from the reference: c_ap, c_max_recall, c_rows; from the restatement: c_tp, c_duplicates
_FIX = {}


def fixture():
    if 'z' not in _FIX:
        _FIX['z'] = dict(np.load(os.path.join(GOLDEN, "sharded_map_ref.npz")))
        _FIX['random'] = dict(np.load(os.path.join(GOLDEN, "voc_map_ref.npz")))
    return _FIX['z']


def load_case(case):
    """-> (images, C, ids, sum_gt, shards) of a case"""
    z = fixture()
    pool, n, world = CASES[case]
    images, C, _ = vnp.load_set(_FIX['random'] if pool == 'random' else z, pool)
    cut = np.concatenate([[0], np.cumsum(z[case + '_shard_counts'])])
    shards = [z[case + '_shards'][cut[r]:cut[r + 1]].tolist() for r in range(world)]
    return images[:n], C, z[case + '_ids'], z[case + '_sum_gt'], shards
