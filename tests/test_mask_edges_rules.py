"""The mask edge suite without a GPU: the numpy statements (tests/mask_rle_np.py, tests/mask_poly_np.py), the host fallback encoder
(scda_amd/mask_rle_host.py) and the host string decode equal what the reference's compiled maskApi.c recorded for every case of
tests/mask_edge_cases.py (tests/golden/mask_edges_ref.npz, tests/golden/make_golden_mask_edges.py); the fixture's inputs are the
table's; and the table still contains the boundary cases it names."""
import os

import numpy as np
import pytest

import mask_edge_cases as E
import mask_poly_np as mp
import mask_rle_np as R


def _groups():
    """-> {prefix: [(name, bool mask)]} of the encoder-shaped groups, the large plane included"""
    bits, info = E.batch300()
    wide, wsz = E.wide_batch()
    return {'wide': [('wide/%d' % r, R.unpack(wide[r], int(wsz[r, 0]), int(wsz[r, 1]))) for r in range(len(wide))],
            'enc': [(c['name'], c['mask']) for c in E.encoder_cases()],
            'b300': [('b300/%d' % r, R.unpack(bits[r], int(info[r // 3, 0]), int(info[r // 3, 1]))) for r in range(300)],
            'hint': [(c['name'], c['mask']) for c in E.hint_cases()],
            'large': [('large', E.large_mask())]}


def test_fixture_inputs_are_the_table_and_it_is_small(golden_dir):
    g = E.fixture(golden_dir)
    enc, hint = E.encoder_cases(), E.hint_cases()
    assert g['enc_name'].tolist() == [c['name'] for c in enc] and g['hint_name'].tolist() == [c['name'] for c in hint]
    assert np.array_equal(g['enc_bits'], np.stack([E.pack(c['mask']) for c in enc]))
    assert np.array_equal(g['enc_size'], [(c['h'], c['w']) for c in enc])
    assert np.array_equal(g['hint_bits'], np.stack([E.pack(c['mask']) for c in hint]))
    assert g['hint_roi'].tobytes() == np.stack([c['roi'] for c in hint]).tobytes()
    bits, info = E.batch300()
    assert np.array_equal(g['b300_bits'], bits) and np.array_equal(g['b300_info'], info)
    bits, info = E.wide_batch()
    assert np.array_equal(g['wide_bits'], bits) and np.array_equal(g['wide_info'], info)
    for i, (h, w) in enumerate(E.IOU_SIZES):
        names, dt, gt = E.iou_masks(h, w, 900 + i)
        key = 'iou_%dx%d' % (h, w)
        assert g[key + '_name'].tolist() == names
        assert np.array_equal(g[key + '_dt'], np.stack([E.pack(m) for m in dt])) and np.array_equal(g[key + '_gt'], np.stack([E.pack(m) for m in gt]))
    dt, gt, crowd = E.iou_m70()
    assert np.array_equal(g['iou_m70_dt'], np.stack([E.pack(m) for m in dt])) and np.array_equal(g['iou_m70_gt'], np.stack([E.pack(m) for m in gt]))
    for prefix, planes in (('poly', E.poly_cases()), ('polybig', E.poly_big_cases())):
        assert g[prefix + '_name'].tolist() == ['' if c is None else c['name'] for c in planes]
        for k, v in E.flat_annotations(planes).items():
            assert g[prefix + '_' + k].dtype == v.dtype and g[prefix + '_' + k].tobytes() == v.tobytes(), (prefix, k)
    # data only, the 4100 x 4100 plane as its outputs, and the bound the project puts on mask_rle_ref.npz
    assert not [k for k in g if k.startswith('large') and g[k].size > 64]
    assert os.path.getsize(os.path.join(golden_dir, "mask_edges_ref.npz")) <= os.path.getsize(
        os.path.join(golden_dir, "predict_masks_sweep.npz"))


@pytest.mark.parametrize("prefix", ('enc', 'wide', 'b300', 'hint', 'large'))
def test_statement_and_host_fallback_equal_the_reference(golden_dir, prefix):
    from scda_amd import mask_rle_host as host
    g = E.fixture(golden_dir)
    cases = _groups()[prefix]
    assert len(cases) == len(g[prefix + '_area'])
    for i, (name, m) in enumerate(cases):
        want = E.recorded(g, prefix, i)
        s = R.statement(m)
        assert s['n_runs'] == want['n_runs'] and np.array_equal(s['counts'], want['counts']), name
        assert s['chars'] == want['chars'] and s['area'] == want['area'] and s['bbox'] == want['bbox'], (name, s['bbox'], want['bbox'])
        assert np.array_equal(host.rle_counts(m), want['counts']), name
        assert host.encode(m) == {'size': list(m.shape), 'counts': want['chars'].decode('ascii'), 'area': want['area'],
                                  'bbox': want['bbox']}, name


def test_numpy_iou_equals_the_reference(golden_dir):
    g = E.fixture(golden_dir)
    for i, (h, w) in enumerate(E.IOU_SIZES):
        _, dt, gt = E.iou_masks(h, w, 900 + i)
        key = 'iou_%dx%d' % (h, w)
        crowd = E.iou_crowd(len(gt))
        for c, o in ((crowd, g[key + '_o0']), (1 - crowd, g[key + '_o1'])):
            got_o, got_i = R.iou(dt, gt, c)
            assert got_o.tobytes() == o.tobytes() and np.array_equal(got_i, g[key + '_inter']), key
    dt, gt, crowd = E.iou_m70()
    got_o, got_i = R.iou(dt, gt, crowd)
    assert got_o.tobytes() == g['iou_m70_o'].tobytes() and np.array_equal(got_i, g['iou_m70_inter'])


@pytest.mark.parametrize("prefix", ('poly', 'polybig'))
def test_polygon_statement_and_string_decode_equal_the_reference(golden_dir, prefix):
    from scda_amd import coco_gt
    g = {k[len(prefix):]: v for k, v in E.fixture(golden_dir).items() if k.startswith(prefix + '_')}
    H, Wd = g['_bits'].shape[1:]
    for n, c in enumerate(E.poly_cases() if prefix == 'poly' else E.poly_big_cases()):
        if c is None:
            assert not g['_bits'][n].any() and g['_area'][n] == 0
            continue
        counts = c['counts']
        if c['string'] is not None:
            assert E.cut(g['_str'], g['_str_first'], n).tobytes() == c['string'], c['name']
            counts = mp.fr_string(c['string'])
            recorded = E.cut(g['_str_counts'], g['_str_counts_first'], n)
            assert np.array_equal(counts, recorded) and np.array_equal(recorded, c['counts']), c['name']
            assert np.array_equal(coco_gt.counts_from_string(c['string']), recorded), c['name']
        got = mp.annotation(c['h'], c['w'], c['polygons'], counts)
        assert np.array_equal(E.pack(got, H, Wd), g['_bits'][n]), c['name']
        assert int(got.sum()) == g['_area'][n], c['name']
        fp = E.cut(g['_frpoly'], g['_frpoly_first'], n)
        if len(c['polygons']) == 1 and c['counts'] is None:
            assert np.array_equal(R.encode(got), fp), c['name']               # rleFrPoly's own counts are canonical
        else:
            assert len(fp) == 0


def test_table_holds_the_cases_it_names(golden_dir):
    g = E.fixture(golden_dir)
    enc = {c['name']: (c, E.recorded(g, 'enc', i)) for i, c in enumerate(E.encoder_cases())}
    for (h, w) in E.ENC_SIZES:                                                # every size has every pattern that fits, both run parities
        tag = '%dx%d/' % (h, w)
        assert enc[tag + 'checker1'][1]['n_runs'] == h * w + 1 and enc[tag + 'checker0'][1]['n_runs'] == max(h * w, 1 + (h * w > 1))
        assert enc[tag + 'empty'][1]['counts'].tolist() == [h * w] and enc[tag + 'full'][1]['counts'].tolist() == [0, h * w]
        assert (tag + 'col31_32' in enc) == (w > 32) and (tag + 'rows31_32' in enc) == (h > 32)
    assert enc['66x96/col31_32'][1]['counts'].tolist() == [31 * 66, 2 * 66, 63 * 66]             # one run over the word boundary
    assert enc['66x96/bottom31'][1]['bbox'] == [31, 65, 1, 1] and enc['66x96/top32'][1]['counts'][0] == 32 * 66
    assert enc['64x64/last'][1]['counts'].tolist() == [4095, 1] and enc['66x96/rows31_32'][1]['n_runs'] == 2 * 96 + 1
    # a column of 32 x 32 blocks with 32 transitions per column, and a block-row carry above 255
    assert enc['66x96/checker0'][0]['mask'].shape == (66, 96) and enc['66x96/checker0'][1]['n_runs'] > 256 * 4
    # six-character differences of both signs
    large = E.recorded(g, 'large', 0)
    x = large['counts'].astype(np.int64); x[3:] -= large['counts'][1:-2].astype(np.int64)
    six = [int(v) for v in x if len(R.to_string(np.array([v]))) == 6]
    assert large['counts'].tolist() == [0, 16800000, 1, 1, 9998] and sorted(six) == [-16799999, 16800000] and len(large['chars']) == 17
    # the hint: a window whose last column is a word's last column and that reaches the last row; a first scanned word that is not
    # word 0; dead windows of every kind with all-zero planes
    hint = {c['name']: c for c in E.hint_cases()}
    c = hint['66x96/win0/full']
    assert int(c['roi'][3]) % 32 == 31 and c['mask'][65, 31] and not c['mask'][:, 32:].any()
    assert hint['66x96/win1/full']['mask'][:, :32].sum() == 0 and hint['66x96/win2/full']['mask'][65, 95]
    for k in (8, 9, 10, 11, 12):
        assert not hint['66x96/win%d/full' % k]['mask'].any(), k
    assert E.trunc(float('nan')) is None and E.trunc(6e8) is None and E.trunc(-3.5) == -3 and E.trunc(63.99) == 63
    assert hint['40x64/win1/full']['mask'][39, 63] and hint['66x70/win2/full']['mask'][65, 69] and hint['66x96/win7/random']['mask'][:, 90:].any()         # past the image's edges
    # IoU: an intersecting pair that the box gate zeroes, identical pairs, M != N
    names = g['iou_66x96_name'].tolist()
    d, t = names.index('wrap'), names.index('two')
    assert g['iou_66x96_inter'][t, d] == 2 and g['iou_66x96_o0'][t, d] == 0.0 and g['iou_66x96_o1'][t, d] == 0.0
    assert g['iou_66x96_o0'][d, d] == 1.0 and g['iou_66x96_o0'].shape == (len(names) - 2, len(names))
    assert g['iou_66x96_inter'][names.index('from31'), names.index('to31')] == 66                       # column 31 alone
    assert g['iou_66x96_inter'][names.index('from32'), names.index('to32')] == 66
    assert g['iou_66x96_inter'][names.index('from31b'), names.index('to32b')] == 2 * 66
    assert g['iou_66x96_inter'][names.index('c32_33'), names.index('c30_31')] == 0
    assert g['iou_32x32_inter'][1, 1] == 1024 and g['iou_m70_o'].shape == (3, 70) and g['iou_m70_o'][2, 41] == 1.0
    assert (g['iou_66x96_o0'] != g['iou_66x96_o1']).any()
    # annToMask: toggles at h * w in a word / uint4 group of its own, run counts of both parities, zero-length runs, scan rounds
    poly = {c['name']: c for c in E.poly_cases() if c is not None}
    for (h, w) in ((32, 32), (64, 64), (4, 32)):
        c = poly['%dx%d/rle/even_exact' % (h, w)]
        assert h * w % 128 == 0 and len(c['counts']) % 2 == 0 and int(c['counts'].sum()) == h * w
        assert len(poly['%dx%d/rle/odd_exact' % (h, w)]['counts']) % 2 == 1
    assert (1 * 32) % 128 == 32 and (33 * 31) % 32 == 31 and (1 * 33) % 32 == 1
    assert len(poly['64x64/rle/runs1100']['counts']) > 4 * 256 and len(poly['66x96/rle/runs600']['counts']) > 256
    assert poly['66x96/rle/zeros_inside']['counts'].tolist().count(0) == 3
    slot = poly['66x96/empty_slot']['polygons']
    assert [len(p) for p in slot] == [4, 0, 3]
    first = g['poly_poly_first']
    assert (np.diff(first) == 0).sum() == len(E.POLY_SIZES)                   # poly_first[p] == poly_first[p + 1]
    u, v = mp.edge_points(0, 0, 5 * 96, 5 * 66)
    assert len(u) == 481 and len(poly['66x96/union']['polygons']) == 3 and poly['66x96/union']['counts'] is not None
    assert sum(c is None for c in E.poly_cases()) == len(E.POLY_SIZES) + 2
    # a fill across the parity scan's round boundary, a column scan of two rounds
    big = E.poly_big_cases()
    assert E.BIG['h'] * E.BIG['w'] > 256 * 128 and big[0]['counts'][0] < 256 * 128 < big[0]['counts'][:2].sum() and big[1] is None
    assert g['polybig_bits'][3].any() and g['wide_info'][:, 1].min() > 256 and (g['wide_area'] > 0).all()
