"""COCO ground-truth masks on the MI355X (scda_amd/csrc/mask_poly.hip, scda_amd/coco_gt.py) against what the reference's compiled
maskApi.c gave (tests/golden/mask_poly_ref.npz), bit for bit: every small case in one batch of planes with different image sizes, the
800 x 1344 cases in a second call, the popcount areas, determinism and the every-word-written rule, empty planes, the loop back through
scda_mask_rle_hip, and evaluate.coco_stats with the ground truth given as packed masks and as annotations."""
import numpy as np
import pytest
import torch

import mask_poly_np as mp
from gpu_arrays import pack as _pack
from scda_amd import coco_gt
from test_mask_poly_rules import annotation_of, fixture_cases

pytestmark = pytest.mark.gpu

EMPTY_AT = (0, 17, 101)                         # images without an annotation, put between the cases: planes that nothing maps to


_RUNS = {}


def _rasterised(cuda, golden_dir, big):
    """the small (or the 800 x 1344) cases of the fixture, one plane each, through native.mask_frpoly TWICE into the same buffers, the
    planes pre-filled with ones -> (cases or None per plane, words of both calls, areas, the device planes).  The flat arrays are laid
    out here and not by flatten_annotations: rleFrPoly takes the one- and two-vertex polygons that COCO.annToRLE never hands to it."""
    from scda_amd import native as N
    if big not in _RUNS:
        planes = [c for c in fixture_cases(golden_dir) if c['big'] == big]
        for i in EMPTY_AT if not big else (1,):
            planes.insert(i, None)
        H, Wd = (800, 42) if big else (40, 3)
        xy, poly_first, poly_plane, counts, rle_first, rle_plane = [], [0], [], [], [0], []
        for n, c in enumerate(planes):
            for p in ([] if c is None else c['polygons']):
                xy.append(p); poly_first.append(poly_first[-1] + len(p)); poly_plane.append(n)
            if c is not None and c['kind']:
                r = c['counts'] if c['kind'] == 1 else coco_gt.counts_from_string(c['string'])
                counts.append(r.view(np.int32)); rle_first.append(rle_first[-1] + len(r)); rle_plane.append(n)
        sizes = [(7, 9) if c is None else (c['h'], c['w']) for c in planes]
        i32 = lambda a: N.upload(np.asarray(a, dtype=np.int32), cuda)         # noqa: E731
        args = (N.upload(np.concatenate(xy), cuda), i32(poly_first), i32(poly_plane), i32(np.concatenate(counts)), i32(rle_first),
                i32(rle_plane), i32(sizes))
        ws = torch.empty(N.mask_frpoly_workspace_bytes(len(poly_plane), len(rle_plane), H, Wd), dtype=torch.uint8, device=cuda)
        bits = torch.full((len(planes), H, Wd), -1, dtype=torch.int32, device=cuda)
        area = torch.full((len(planes),), -1, dtype=torch.int32, device=cuda)
        words = []
        for _ in range(2):
            assert N.mask_frpoly(*args, ws, bits, area=area) is bits
            words.append(bits.cpu().numpy().view(np.uint32).copy())
        _RUNS[big] = (planes, words, area.cpu().numpy().view(np.uint32), bits)
    return _RUNS[big]


@pytest.mark.parametrize("big", (False, True), ids=("small", "800x1344"))
def test_planes_equal_the_reference_bit_for_bit(cuda, golden_dir, big):
    planes, words, area, _ = _rasterised(cuda, golden_dir, big)
    H, Wd = words[0].shape[1:]
    bad = {}
    for n, c in enumerate(planes):
        want = np.zeros((H, Wd), np.uint32) if c is None else _pack(mp.decode_counts(c['runs'], c['h'], c['w']), H, Wd)
        if not np.array_equal(words[0][n], want):                             # the whole plane: zero bits outside the image included
            g = 'empty' if c is None else c['group']
            bad.setdefault(g, []).append(n)
    assert not bad, bad
    assert {c['group'] for c in planes if c is not None} == (set('ij') if big else set('abcdefghi'))


@pytest.mark.parametrize("big", (False, True), ids=("small", "800x1344"))
def test_areas_equal_rle_area(cuda, golden_dir, big):
    planes, _, area, _ = _rasterised(cuda, golden_dir, big)
    assert area.tolist() == [0 if c is None else c['area'] for c in planes]


@pytest.mark.parametrize("big", (False, True), ids=("small", "800x1344"))
def test_a_second_call_gives_identical_bytes_and_every_word_is_written(cuda, golden_dir, big):
    planes, words, _, _ = _rasterised(cuda, golden_dir, big)                  # the planes were all ones before the first call
    assert words[0].tobytes() == words[1].tobytes()
    for n, c in enumerate(planes):
        if c is None:                                                         # planes that nothing maps to are empty
            assert not words[0][n].any(), n


def test_mask_rle_gives_back_the_counts_of_rle_fr_poly(cuda, golden_dir):
    from scda_amd import native as N
    planes, _, _, bits = _rasterised(cuda, golden_dir, False)
    single = [n for n, c in enumerate(planes) if c is not None and len(c['frpoly'])]
    assert len(single) > 200
    sizes = torch.tensor([[planes[n]['h'], planes[n]['w']] for n in single], dtype=torch.float32, device=cuda)
    got = N.mask_rle(bits[single].contiguous(), image_info=sizes, cap_runs=max(len(planes[n]['frpoly']) for n in single))
    n_runs, counts = got['n_runs'].cpu().numpy(), got['counts'].cpu().numpy().view(np.uint32)
    for r, n in enumerate(single):
        want = planes[n]['frpoly']
        assert n_runs[r] == len(want) and np.array_equal(counts[r, :len(want)], want), (n, planes[n]['group'])


def test_raw_entry_point_takes_no_shape_at_all(cuda):
    from scda_amd import native as N
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=cuda).reshape(-1)          # noqa: E731
    out = torch.full((2, 5, 1), -1, dtype=torch.int32, device=cuda)
    area = torch.full((2,), -1, dtype=torch.int32, device=cuda)
    ws = torch.empty(N.mask_frpoly_workspace_bytes(0, 0, 5, 1), dtype=torch.uint8, device=cuda)
    N.mask_frpoly(torch.zeros(0, 2, dtype=torch.float64, device=cuda), i32(0), i32(), i32(), i32(0), i32(), i32(5, 7, 3, 32).reshape(2, 2),
                  ws, out, area=area)
    assert not out.any() and not area.any()
    with pytest.raises(ValueError):
        N.mask_frpoly(torch.zeros(0, 2, dtype=torch.float64, device=cuda), i32(0), i32(), i32(), i32(0), i32(), i32(5, 7).reshape(1, 2),
                      ws, out)                                                # sizes of another N


class _StandIn:
    """what evaluate.coco_stats reads of a Predictor(masks=True, rle=True): the flags and the call"""
    masks = rle = True

    def __init__(self, outs):
        self.outs = list(outs)

    def __call__(self, image, image_info):
        return self.outs.pop(0)


def _synthetic(golden_dir, cuda, H, Wd, D, K):
    """three images (37 x 70, 5 x 33 and the size of the first duplicated-vertex pair) whose ground truth is the fixture's cases of that
    size -- polygons, counts and strings -- and whose detections are seeded rectangles and those masks shifted by a pixel, with seeded
    scores and categories"""
    from scda_amd import infer
    cases = fixture_cases(golden_dir)
    rng = np.random.RandomState(9)
    images = []
    pair = next(c for c in cases if c['group'] == 'e')
    for size in ((37, 70), (5, 33), (pair['h'], pair['w'])):
        gts = [c for c in cases if (c['h'], c['w']) == size and c['group'] in 'efhi']
        assert 2 <= len(gts) <= 16
        anns = [annotation_of(c, category_id=1 + g % K, iscrowd=int(g % 5 == 4)) for g, c in enumerate(gts)]
        masks = [mp.decode_counts(c['runs'], *size) for c in gts]
        det = np.zeros((D, 7), np.float32)
        dmask = np.zeros((D,) + size, bool)
        boxes = []
        for _ in range(3):                                                    # seeded rectangles, whatever the ground truth is
            y0, x0 = rng.randint(size[0]), rng.randint(size[1])
            m = np.zeros(size, bool); m[y0:y0 + 1 + rng.randint(size[0]), x0:x0 + 1 + rng.randint(size[1])] = True
            boxes.append((m, 1 + rng.randint(K)))
        shifted = [(np.roll(m, shift, axis=(0, 1)), anns[g]['category_id'] if rng.rand() < 0.8 else 1 + rng.randint(K))
                   for g, m in enumerate(masks) for shift in ((0, 1), (1, 0))]
        n = 0
        for d, cat in boxes + shifted:
            ys, xs = np.nonzero(d)
            if not len(ys):
                continue
            dmask[n] = d
            det[n, 1:5] = (xs.min(), ys.min(), xs.max(), ys.max())
            det[n, 5], det[n, 6] = np.round(rng.uniform(0.05, 1), 2), cat
            n += 1
        assert 3 <= n <= D
        planes = np.zeros((D, H, Wd * 32), bool)
        planes[:, :size[0], :size[1]] = dmask
        images.append({'size': size, 'anns': anns, 'gt_masks': masks, 'det': det, 'n': n, 'bits': infer.pack_masks(planes),
                       'area': dmask.reshape(D, -1).sum(1).astype(np.int32)})
    return images


def _items(images, idx, form, G, H, Wd, cuda):
    from scda_amd import infer
    B = len(idx)
    det = np.stack([images[i]['det'] for i in idx]); det[:, :, 0] = np.arange(B)[:, None]
    out = (None, None, torch.from_numpy(det).to(cuda), torch.tensor([images[i]['n'] for i in idx], dtype=torch.int32, device=cuda),
           torch.stack([images[i]['bits'] for i in idx]).to(cuda), {'area': torch.from_numpy(np.stack([images[i]['area'] for i in idx])).to(cuda)})
    item = {'image': torch.zeros(B, 3, 8, 8), 'image_info': None, 'image_ids': torch.tensor([40 + i for i in idx], dtype=torch.int32),
            'sizes': [images[i]['size'] for i in idx]}
    if form == 'annotations':
        item['annotations'] = [images[i]['anns'] for i in idx]
    else:
        flat = coco_gt.flatten_annotations([images[i]['anns'] for i in idx], item['sizes'], G)
        item.update({k: torch.from_numpy(flat[k]) for k in ('gt_boxes', 'gt_areas', 'gt_iscrowd', 'gt_categories', 'gt_counts')})
        dense = np.zeros((B, G, H, Wd * 32), bool)
        for b, i in enumerate(idx):
            h, w = images[i]['size']
            for g, m in enumerate(images[i]['gt_masks']):
                dense[b, g, :h, :w] = m                                       # the golden dense masks
        item['gt_mask_bits'] = infer.pack_masks(dense.reshape(B * G, H, Wd * 32)).reshape(B, G, H, Wd)
    return out, item


def test_coco_stats_from_annotations_equal_those_from_packed_masks(cuda, golden_dir):
    from scda_amd import evaluate
    from scda_amd.coco_eval import CocoEvaluator
    H, Wd, D, G, K = 40, 3, 32, 16, 3
    images = _synthetic(golden_dir, cuda, H, Wd, D, K)
    stats = {}
    for form in ('gt_mask_bits', 'annotations'):
        pairs = [_items(images, idx, form, G, H, Wd, cuda) for idx in ([0, 1], [2])]
        ev = CocoEvaluator(K, 'segm', max_images=3, max_dets_per_image=D, max_gts_per_image=G, device=cuda,
                           params={'area_rng': [[0, 1e10], [0, 60], [60, 400], [400, 1e10]]})
        stats[form] = evaluate.coco_stats([p[1] for p in pairs], _StandIn(p[0] for p in pairs), ev)
    print("stats", stats['annotations'])
    assert stats['annotations'].dtype == np.float64 and stats['annotations'].shape == (12,)
    assert stats['annotations'].tobytes() == stats['gt_mask_bits'].tobytes()
    assert stats['annotations'][0] > 0
    # a 'bbox' evaluator takes the annotations as well (no mask is rasterised)
    for form in ('gt_mask_bits', 'annotations'):
        pairs = [_items(images, idx, form, G, H, Wd, cuda) for idx in ([0, 1, 2],)]
        ev = CocoEvaluator(K, 'bbox', max_images=3, max_dets_per_image=D, max_gts_per_image=G, device=cuda)
        stats[form] = evaluate.coco_stats([p[1] for p in pairs], _StandIn(p[0] for p in pairs), ev)
    assert stats['annotations'].tobytes() == stats['gt_mask_bits'].tobytes()
