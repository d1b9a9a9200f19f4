"""The rule of scda_mask_frpoly_hip without a GPU: the numpy statement (tests/mask_poly_np.py) against what the reference's compiled
maskApi.c gave (tests/golden/mask_poly_ref.npz, every case), the host half of scda_amd.coco_gt (flatten_annotations: the three
segmentation forms, the reference's skips, the refused inputs) and the compressed-string decode."""
import os

import numpy as np
import pytest

import mask_poly_np as mp
from scda_amd import coco_gt

_CASES = {}


def fixture_cases(golden_dir):
    """-> list of dicts: group, h, w, polygons [float64 [k, 2]], kind (0 polygons, 1 counts, 2 string), counts, string, runs (the
    decoded mask's run counts), area, frpoly (rleFrPoly's own counts of a single-polygon case)"""
    if golden_dir not in _CASES:
        z = np.load(os.path.join(golden_dir, "mask_poly_ref.npz"))
        cut = lambda name, first, i: z[name][z[first][i]:z[first][i + 1]]     # noqa: E731
        cases = []
        for i in range(len(z['group'])):
            polys = [cut('xy', 'vert_first', p) for p in range(z['poly_first'][i], z['poly_first'][i + 1])]
            cases.append({'group': str(z['group'][i]), 'h': int(z['size'][i, 0]), 'w': int(z['size'][i, 1]), 'big': bool(z['big'][i]),
                          'polygons': polys, 'kind': int(z['kind'][i]), 'counts': cut('rle_counts', 'rle_first', i),
                          'string': cut('str_bytes', 'str_first', i).tobytes(), 'runs': cut('out_counts', 'out_first', i),
                          'area': int(z['area'][i]), 'frpoly': cut('frpoly_counts', 'frpoly_first', i)})
        _CASES[golden_dir] = cases
    return _CASES[golden_dir]


def annotation_of(case, category_id=1, iscrowd=0):
    """the case as a COCO annotation dict (box and area from the recorded mask)"""
    if case['kind'] == 0:
        segm = [p.reshape(-1).tolist() for p in case['polygons']]
    elif case['kind'] == 1:
        segm = {'size': [case['h'], case['w']], 'counts': case['counts'].tolist()}
    else:
        segm = {'size': [case['h'], case['w']], 'counts': case['string'].decode()}
    m = mp.decode_counts(case['runs'], case['h'], case['w'])
    ys, xs = np.nonzero(m)
    box = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)] if len(ys) else [0.0] * 4
    return {'segmentation': segm, 'bbox': box, 'area': float(m.sum()), 'iscrowd': iscrowd, 'category_id': category_id}


def test_the_fixture_holds_every_group(golden_dir):
    cases = fixture_cases(golden_dir)
    n = {g: sum(c['group'] == g for c in cases) for g in 'abcdefghij'}
    assert n['a'] >= 200 and n['e'] >= 10 and n['g'] >= 6 and n['h'] >= 8 and n['i'] >= 8 and n['j'] == 2 and min(n.values()) >= 1, n
    assert {(c['h'], c['w']) for c in cases if c['group'] == 'f'} == {(5, 33), (37, 70)}
    assert all((c['h'], c['w']) == (800, 1344) for c in cases if c['group'] == 'j')
    # group e: a duplicated vertex changes the recorded mask of its twin
    e = [c for c in cases if c['group'] == 'e']
    assert all(not np.array_equal(e[i]['runs'], e[i + 1]['runs']) for i in range(0, len(e), 2))


def test_statement_equals_the_reference_on_every_case(golden_dir):
    for i, c in enumerate(fixture_cases(golden_dir)):
        counts = None if c['kind'] == 0 else c['counts'] if c['kind'] == 1 else mp.fr_string(c['string'])
        got = mp.annotation(c['h'], c['w'], c['polygons'], counts)
        want = mp.decode_counts(c['runs'], c['h'], c['w'])
        assert np.array_equal(got, want), (i, c['group'], int((got != want).sum()))
        assert int(got.sum()) == c['area'], (i, c['group'])


def test_string_decode_equals_the_recorded_counts(golden_dir):
    strings = [c for c in fixture_cases(golden_dir) if c['kind'] == 2]
    assert strings
    for c in strings:
        for s in (c['string'], c['string'].decode()):
            got = coco_gt.counts_from_string(s)
            assert got.dtype == np.uint32 and np.array_equal(got, c['counts']), c['string']
        assert np.array_equal(mp.fr_string(c['string']), c['counts'])
    # differences of 1 .. 5 characters and negative ones occur
    big = next(c for c in strings if c['big'])['counts'].astype(np.int64)
    diff = big.copy(); diff[3:] -= big[1:-2]
    assert diff.min() < -2 ** 14 and diff.max() >= 2 ** 19
    with pytest.raises(ValueError):
        coco_gt.counts_from_string(b'0P')                                     # ends inside a value


def _rebuilt(flat, n, h, w):
    """plane n of flatten_annotations' arrays through the numpy statement"""
    polys = [flat['xy'][flat['poly_first'][p]:flat['poly_first'][p + 1]] for p in np.flatnonzero(flat['poly_plane'] == n)]
    m = mp.annotation(h, w, polys)
    for q in np.flatnonzero(flat['rle_plane'] == n):
        m |= mp.annotation(h, w, (), flat['rle_counts'][flat['rle_first'][q]:flat['rle_first'][q + 1]])
    return m


def test_flatten_round_trips_the_three_forms(golden_dir):
    cases = fixture_cases(golden_dir)
    sizes = sorted({(c['h'], c['w']) for c in cases if c['group'] in 'fghi' and not c['big']})
    images = [[c for c in cases if (c['h'], c['w']) == s and c['group'] in 'fghi'] for s in sizes]
    assert {c['kind'] for im in images for c in im} == {0, 1, 2}
    gcap = max(len(im) for im in images) + 1
    flat = coco_gt.flatten_annotations([[annotation_of(c, category_id=3 + g, iscrowd=g % 2) for g, c in enumerate(im)] for im in images],
                                       sizes, gcap, plane=(40, 3))
    B = len(images)
    assert flat['xy'].dtype == np.float64 and flat['rle_counts'].dtype == np.uint32 and flat['sizes'].shape == (B * gcap, 2)
    for k in ('poly_first', 'poly_plane', 'rle_first', 'rle_plane', 'sizes', 'gt_categories', 'gt_counts'):
        assert flat[k].dtype == np.int32, k
    assert (np.diff(flat['poly_plane']) >= 0).all() and (np.diff(flat['rle_plane']) >= 0).all()
    assert flat['gt_counts'].tolist() == [len(im) for im in images]
    for b, im in enumerate(images):
        h, w = sizes[b]
        assert (flat['sizes'][b * gcap:(b + 1) * gcap] == (h, w)).all()
        for g, c in enumerate(im):
            want = mp.decode_counts(c['runs'], h, w)
            assert np.array_equal(_rebuilt(flat, b * gcap + g, h, w), want), (b, g, c['group'])
            assert flat['gt_areas'][b, g] == c['area'] and flat['gt_categories'][b, g] == 3 + g and flat['gt_iscrowd'][b, g] == g % 2
            assert flat['gt_boxes'][b, g].tolist() == annotation_of(c)['bbox']
        assert not _rebuilt(flat, b * gcap + len(im), h, w).any()             # a slot that nothing maps to
        assert not flat['gt_areas'][b, len(im):].any()


def test_flatten_keeps_the_reference_skips():
    ann = {'bbox': [0, 0, 1, 1], 'area': 1.0, 'iscrowd': 0, 'category_id': 1}
    poly = [1.0, 1.0, 8.0, 2.0, 5.0, 7.0]
    a = coco_gt.flatten_annotations([[dict(ann, segmentation=[poly + [3.5]])]], (10, 12), 2)      # a trailing odd value is dropped
    b = coco_gt.flatten_annotations([[dict(ann, segmentation=[poly])]], (10, 12), 2)
    assert np.array_equal(a['xy'], b['xy']) and a['poly_first'].tolist() == [0, 3]
    e = coco_gt.flatten_annotations([[dict(ann, segmentation=[])], []], (10, 12), 2)              # no polygon: an empty mask
    assert e['xy'].shape == (0, 2) and e['poly_first'].tolist() == [0] and e['gt_counts'].tolist() == [1, 0]
    assert e['rle_counts'].shape == (0,) and e['rle_first'].tolist() == [0] and e['sizes'].tolist() == [[10, 12]] * 4


@pytest.mark.parametrize("bad", ("too_many", "size_zero", "size_outside", "planes", "rows", "pixels", "nan", "inf", "far", "rle_sum", "rle_size",
                                 "string_sum", "box"))
def test_flatten_refuses_what_the_kernels_do_not_take(bad):
    ann = {'bbox': [0, 0, 1, 1], 'area': 1.0, 'iscrowd': 0, 'category_id': 1, 'segmentation': [[1.0, 1.0, 8.0, 2.0, 5.0, 7.0]]}
    anns, sizes, gcap, plane = [[ann]], (10, 12), 2, (16, 1)
    assert coco_gt.flatten_annotations(anns, sizes, gcap, plane=plane)['poly_plane'].tolist() == [0]
    seg = lambda s: [[dict(ann, segmentation=s)]]                             # noqa: E731
    if bad == "too_many":
        anns = [[ann, ann, ann]]
    elif bad == "size_zero":
        sizes = (0, 12)
    elif bad == "size_outside":
        sizes = (10, 33)
    elif bad == "planes":
        anns, gcap = [[ann]] * 2, 32768
    elif bad == "rows":
        plane = (65536, 1)
    elif bad == "pixels":
        plane = (65535, 1025)
    elif bad == "nan":
        anns = seg([[1.0, float('nan'), 8.0, 2.0, 5.0, 7.0]])
    elif bad == "inf":
        anns = seg([[1.0, 1.0, float('inf'), 2.0, 5.0, 7.0]])
    elif bad == "far":
        anns = seg([[1.0, 1.0, 8.0, -65536.0, 5.0, 7.0]])
    elif bad == "rle_sum":
        anns = seg({'size': [10, 12], 'counts': [100, 21]})
    elif bad == "rle_size":
        anns = seg({'size': [12, 10], 'counts': [100, 20]})
    elif bad == "string_sum":
        anns = seg({'size': [10, 12], 'counts': '0' + chr(48 + 0x20 + 25) + chr(48 + 3)})          # runs 0, 121
    else:
        anns = seg([[1.0, 1.0, 8.0, 7.0]])                                    # four values: a box to the reference
    with pytest.raises(ValueError):
        coco_gt.flatten_annotations(anns, sizes, gcap, plane=plane)
