"""Generates tests/golden/sharded_map_ref.npz with the REFERENCE's metric over sharded validation: utils/cal_mAP.py is imported
UNMODIFIED (parse_gts, parse_res, cal_mAP), the way make_golden_voc_map.py does, whose text_rows, meta_lines, random_set and
_NumpyEmptyMax are reused by import.  Run in the build container:
    python tests/golden/make_golden_sharded_map.py [path of the reference checkout]

Per case the images are sharded with torch.utils.data.DistributedSampler(range(n), num_replicas=W, rank=r, shuffle=True), epoch 0;
every rank's text rows are written as validate() writes them and concatenated in the order of sorted(str(r) for r in range(W)) -- what
`cat results.txt.rank*` gives --, then parsed and scored by the reference.  Recorded: ap, max_recall, the per-class row counts, the
shard index lists, and the per-row tp of tests/sharded_map_np.py AFTER its ap / max_recall were asserted bit-equal to the reference's.
No reference program text is kept; the file holds inputs and recorded outputs only (layout: tests/sharded_map_np.py).

The cases (sharded_map_np.CASES): the 40 random images of voc_map_ref.npz at 2, 3 and 8 ranks (3 pads; 40 = 5 * 8 does not); their first 7
at 11 ranks (four shards are empty before the padding; the rank order 0, 1, 10, 2, ... matters; with 7 images the sampler puts no
image on more than two ranks, so:) 3 hand-made images at 8 ranks (every image on two or three ranks); hand-made images with one or two detections each whose merged count is 255, 256, 257 and 258 -- 257 is prime, so
under the sampler only one rank gives it; in the 258 case the ids are laid out so that the one repeated image's two positions are the
256th and 257th in id order, across the 256-position round of the duplicate marking --; and a case whose repeated image has no
detection.  main asserts the preconditions that keep the tests from passing vacuously."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_voc_map as mg  # noqa: E402
import sharded_map_np as snp  # noqa: E402


def hand_image(j, detections=True):
    """one ground truth of class 1 (every 7th image: one of class 2 too), found exactly by the first detection; odd images add a
    false positive; scores repeat across images, so the image order decides the ties"""
    gt = [mg.grid_gt(j % 160, 1)]
    det = [tuple(gt[0][:4]) + (.3 + .01 * (j % 50), 1)]
    if j % 2:
        det.append((300, 5, 330, 30, .3 + .01 * ((j + 3) % 50), 1))
    if j % 7 == 0:
        gt.append([340, 100, 379, 139, 2])
        det.append((340, 100, 379, 141, .5 + .01 * (j % 9), 2))
    return {'name': 'h%03d' % j, 'info': mg.f32(200, 400, 1.0), 'gt': np.asarray(gt, dtype=np.int32).reshape(-1, 5),
            'det': mg.det_rows(det if detections else [])}


def pool_arrays(name, images, C):
    out = {'C': np.int64(C), 'names': np.asarray([im['name'] for im in images]), 'info': np.stack([im['info'] for im in images]),
           'det': np.concatenate([im['det'] for im in images]), 'det_counts': np.asarray([len(im['det']) for im in images], dtype=np.int32),
           'gt': np.concatenate([im['gt'] for im in images]).astype(np.int32),
           'gt_counts': np.asarray([len(im['gt']) for im in images], dtype=np.int32)}
    return {name + '_' + k: v for k, v in out.items()}


def reference(cal, images, ids, C, shards, order):
    """the reference over the rank files concatenated in `order` -> ap, max_recall, per-class row counts, the meta's counts"""
    by_position = sorted(range(len(images)), key=lambda i: ids[i])
    meta = mg.meta_lines([(images[i]['name'], images[i]['gt']) for i in by_position])
    rows = [t for r in order for i in shards[r] for t in mg.text_rows(images[i], C)]
    gts, results = cal.parse_gts(meta, C), cal.parse_res(rows)
    cal.np = mg._NumpyEmptyMax()
    try:
        with np.errstate(divide='ignore', invalid='ignore'):
            ap, max_recall = cal.cal_mAP(gts, results, C, 0.5)
    finally:
        cal.np = np
    return np.asarray(ap), np.asarray(max_recall), np.asarray([len(results[c]) if c else 0 for c in range(C)], dtype=np.int32), \
        np.asarray(gts['num']).astype(np.int64)


def main():
    if len(sys.argv) > 1:
        os.environ["SCDA_REFERENCE"] = sys.argv[1]
    import ref_harness
    cal = mg.load_cal_map(ref_harness.REF)
    out = {}
    random_images, _, random_C = mg.random_set()
    hand = [hand_image(j) for j in range(257)]
    zero_first = snp.shard_indices(5, 4)[0][0]                               # the sampler's first index: the first image it repeats
    zero = [hand_image(j, detections=j != zero_first) for j in range(5)]
    out.update(pool_arrays('hand', hand, 3))
    out.update(pool_arrays('zero', zero, 3))
    pools = {'random': (random_images, random_C), 'hand': (hand, 3), 'zero': (zero, 3)}
    for case, (pool, n, W) in snp.CASES.items():
        images, C = pools[pool][0][:n], pools[pool][1]
        shards = snp.shard_indices(n, W)
        ids = np.arange(n, dtype=np.int32)
        if case == 'h258':                                                   # the repeated image at the 256th and 257th place in id order
            rep = shards[0][0]
            ids[[i for i in range(n) if i != rep]] = [k for k in range(n) if k != 255]
            ids[rep] = 255
        order = snp.merge_order(W)
        merged = snp.merged_images(shards, order)
        assert len(merged) == -(-n // W) * W and sorted(set(merged)) == list(range(n))
        ap, max_recall, nrows, sum_gt = reference(cal, images, ids, C, shards, order)
        mine = snp.evaluate_merged(images, merged, ids, C, sum_gt)
        assert mine['ap'].tobytes() == ap.tobytes() and mine['max_recall'].tobytes() == max_recall.tobytes(), (case, mine['ap'], ap)
        assert np.array_equal(mine['rows'], nrows) and mine['duplicates'] == len(merged) - n
        assert np.all(np.isfinite(ap)) and np.all(ap[1:] > 0), (case, ap)
        if case in snp.PADDED:
            # a repeated image whose first copy has a true positive; and the rule matters: keeping the ranks' own tp gives another ap
            firsts = {int(f) for f in mine['first'] if f >= 0}
            local = snp.evaluate_merged(images, merged, ids, C, sum_gt, duplicates='local')
            cut = np.concatenate([[0], np.cumsum([len(images[i]['det']) for i in merged])])
            assert any(mine['tp'][cut[p]:cut[p + 1]].any() for p in firsts), case
            assert local['ap'].tobytes() != ap.tobytes(), case
        else:
            assert mine['duplicates'] == 0
        if case == 'w11':
            assert order != list(range(W)) and any(len(s) == 1 for s in shards) and n < W
            numeric = reference(cal, images, ids, C, shards, list(range(W)))[0]
            assert any(numeric[c].tobytes() != ap[c].tobytes() for c in range(1, C)), "the rank order does not show in any class's ap"
            out[case + '_ap_numeric'] = numeric
        if case == 'few':
            assert max(merged.count(i) for i in range(n)) >= 3
        if case == 'h258':
            place = sorted(range(len(merged)), key=lambda p: (ids[merged[p]], p))
            assert merged[place[255]] == merged[place[256]] and mine['first'][place[256]] == place[255]
        if case == 'zero':
            assert len(images[shards[0][0]]['det']) == 0 and merged.count(shards[0][0]) == 2
        if case[0] == 'h':
            assert len(merged) == int(case[1:]) and all(1 <= len(im['det']) <= 3 for im in images)
        out.update({case + '_ids': ids, case + '_sum_gt': sum_gt, case + '_shards': np.asarray(sum(shards, []), dtype=np.int32),
                    case + '_shard_counts': np.asarray([len(s) for s in shards], dtype=np.int32), case + '_ap': ap,
                    case + '_max_recall': max_recall, case + '_rows': nrows, case + '_tp': mine['tp'],
                    case + '_duplicates': np.int64(mine['duplicates'])})
        print(case, "merged", len(merged), "duplicates", mine['duplicates'], "mAP", np.mean(ap[1:]))
    # the pool 'random' is the one voc_map_ref.npz holds
    with np.load(os.path.join(HERE, "voc_map_ref.npz")) as z:
        assert z['random_det'].tobytes() == np.concatenate([im['det'] for im in random_images]).tobytes()
    path = os.path.join(HERE, "sharded_map_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
