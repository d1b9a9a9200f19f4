"""The run-length, mask-IoU and polygon-fill kernels (scda_amd/csrc/mask_rle.hip, mask_poly.hip) at their edges on the MI355X: the case
table of tests/mask_edge_cases.py -- row-block, word, uint4-group and scan-round boundaries, bits set outside the image, RoI hint
windows of every kind, six-character counts, capacities of one run, unequal IoU set sizes, toggles at h * w, empty polygon slots --
against what the reference's compiled maskApi.c recorded (tests/golden/mask_edges_ref.npz) AND the numpy statements, bit for bit, and
the inputs the reference does not define against what include/scda_ops.h states for them.  Every comparison is equality."""
import numpy as np
import pytest
import torch

import mask_edge_cases as E
import mask_poly_np as mp
import mask_rle_np as R
from gpu_arrays import check_mask, dev, dev_words, host, words

pytestmark = pytest.mark.gpu

GUARD32, GUARD8 = 0x5a5a5a5a, 0x5a


def _check_both(got, r, g, prefix, i, mask, where):
    check_mask(got, r, E.recorded(g, prefix, i), (where, 'fixture'))
    check_mask(got, r, R.statement(mask), (where, 'statement'))


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("form", ("image_info", "info_column", "size"))
def test_encoder_cases_clean_and_dirty(cuda, golden_dir, form):
    """every case twice, zero and ALL ones outside its image: image_info rows, (h, w) in columns 3..4 of wider rows, one size per call"""
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    cases = E.encoder_cases()
    n = len(cases)
    planes = np.stack([E.pack(c['mask']) for c in cases] + [E.pack(c['mask'], dirty=True) for c in cases])
    sizes = np.array([(c['h'], c['w']) for c in cases] * 2, dtype=np.float32)
    cap = int(np.diff(g['enc_first']).max())
    if form == "size":
        for (h, w) in E.ENC_SIZES:
            idx = [i for i in range(2 * n) if tuple(sizes[i]) == (h, w)]
            got = host(N.mask_rle(dev_words(planes[idx], cuda), size=(h, w), cap_runs=h * w + 1))
            for r, i in enumerate(idx):
                _check_both(got, r, g, 'enc', i % n, cases[i % n]['mask'], (form, cases[i % n]['name'], i >= n))
        return
    if form == "image_info":
        got = N.mask_rle(dev_words(planes, cuda), image_info=dev(sizes, cuda), cap_runs=cap)
    else:
        info = np.concatenate([np.full((2 * n, 3), 7.0e8, np.float32), sizes, np.full((2 * n, 1), np.nan, np.float32)], 1)
        got = N.mask_rle(dev_words(planes, cuda), image_info=dev(info, cuda), info_column=3, cap_runs=cap)
    got = host(got)
    for i in range(2 * n):
        _check_both(got, i, g, 'enc', i % n, cases[i % n]['mask'], (form, cases[i % n]['name'], 'dirty' if i >= n else 'clean'))


def test_batches_of_one_of_300_and_of_wide_planes(cuda, golden_dir):
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    cases = E.encoder_cases()
    i = [c['name'] for c in cases].index('65x95/random')
    got = host(N.mask_rle(dev_words(E.pack(cases[i]['mask'], dirty=True)[None], cuda), size=(65, 95), cap_runs=65 * 95 + 1))   # R = 1
    _check_both(got, 0, g, 'enc', i, cases[i]['mask'], 'R = 1')
    bits, info = E.batch300()
    got = host(N.mask_rle(dev_words(bits, cuda), image_info=dev(info, cuda), cap_runs=97))
    assert got['counts'].shape == (300, 97)
    for r in range(300):
        _check_both(got, r, g, 'b300', r, R.unpack(bits[r], int(info[r // 3, 0]), int(info[r // 3, 1])), ('b300', r))
    bits, info = E.wide_batch()
    got = host(N.mask_rle(dev_words(bits, cuda), image_info=dev(info, cuda), cap_runs=3 * 320 + 1))
    for r in range(len(bits)):
        _check_both(got, r, g, 'wide', r, R.unpack(bits[r], int(info[r, 0]), int(info[r, 1])), ('wide', r))


def test_hinted_call_equals_the_unhinted_call_on_every_window(cuda, golden_dir):
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    cases = E.hint_cases()
    n = len(cases)
    bits = dev_words(np.stack([E.pack(c['mask']) for c in cases]), cuda)
    info = dev(np.array([(c['h'], c['w']) for c in cases], dtype=np.float32), cuda)
    rois = dev(np.stack([c['roi'] for c in cases]), cuda)
    cap = int(np.diff(g['hint_first']).max())
    cb = cap * N.mask_rle_max_chars(E.H, E.W)

    def fresh():                                # the unwritten tails are equal as well: both calls start from the same bytes
        i = dict(dtype=torch.int32, device=cuda)
        return {'n_runs': torch.zeros(n, **i), 'counts': torch.zeros(n, cap, **i), 'n_bytes': torch.zeros(n, **i),
                'chars': torch.zeros(n, cb, dtype=torch.uint8, device=cuda), 'area': torch.zeros(n, **i), 'bbox': torch.zeros(n, 4, **i)}
    plain = N.mask_rle(bits, image_info=info, cap_runs=cap, out=fresh())
    hinted = N.mask_rle(bits, image_info=info, rois=rois, cap_runs=cap, out=fresh())
    for k in plain:
        same = (plain[k] == hinted[k]).reshape(n, -1).all(1).cpu().numpy()
        assert same.all(), (k, [cases[i]['name'] for i in np.flatnonzero(~same)])
    gp, gh = host(plain), host(hinted)
    for i, c in enumerate(cases):
        _check_both(gp, i, g, 'hint', i, c['mask'], (c['name'], 'plain'))
        _check_both(gh, i, g, 'hint', i, c['mask'], (c['name'], 'hinted'))


def test_six_character_counts_on_4100x4100(cuda, golden_dir):
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    h, w, Wd = E.LARGE['h'], E.LARGE['w'], E.LARGE['Wd']
    mask = E.large_mask()
    assert N.mask_rle_max_chars(h, 32 * Wd) == 6
    got = host(N.mask_rle(dev_words(E.pack(mask, h, Wd, dirty=True)[None], cuda), size=(h, w), cap_runs=5))
    assert got['chars'].shape == (1, 30) and int(got['n_bytes'][0]) == 17
    _check_both(got, 0, g, 'large', 0, mask, 'large')


def test_capacity_of_one_run_and_of_exactly_the_checkerboard(cuda, golden_dir):
    """guard words in front of and behind counts and chars, as test_capacity_is_exact_and_nothing_is_written_past_it lays them out"""
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    cases = E.encoder_cases()
    names = [c['name'] for c in cases]
    idx = [names.index('66x96/' + k) for k in ('empty', 'checker1', 'checker0', 'first')]
    runs = np.array([E.recorded(g, 'enc', i)['n_runs'] for i in idx])
    assert runs.tolist() == [1, 66 * 96 + 1, 66 * 96, 3]
    bits = dev_words(np.stack([E.pack(cases[i]['mask'], dirty=True) for i in idx]), cuda)
    n = len(idx)
    for cap in (1, int(runs[1]), int(runs[1]) - 1):
        cb = cap * N.mask_rle_max_chars(E.H, E.W)
        cbuf = torch.full((n * cap + 2,), GUARD32, dtype=torch.int32, device=cuda)
        sbuf = torch.full((n * cb + 32,), GUARD8, dtype=torch.uint8, device=cuda)
        out = {'n_runs': torch.empty(n, dtype=torch.int32, device=cuda), 'counts': cbuf[1:1 + n * cap].view(n, cap),
               'n_bytes': torch.empty(n, dtype=torch.int32, device=cuda), 'chars': sbuf[16:16 + n * cb].view(n, cb),
               'area': torch.empty(n, dtype=torch.int32, device=cuda), 'bbox': torch.empty(n, 4, dtype=torch.int32, device=cuda)}
        N.mask_rle(bits, size=(E.H, E.W), cap_runs=cap, out=out)
        got = host(out)
        assert int(cbuf[0]) == GUARD32 and int(cbuf[-1]) == GUARD32, cap
        assert bool((sbuf[:16] == GUARD8).all()) and bool((sbuf[-16:] == GUARD8).all()), cap
        assert np.array_equal(got['n_runs'], runs), cap                       # the true count, also beyond the capacity
        for r, i in enumerate(idx):
            want = E.recorded(g, 'enc', i)
            assert int(got['area'][r].view(np.uint32)) == want['area'] and got['bbox'][r].tolist() == want['bbox'], (cap, names[i])
            if runs[r] <= cap:
                _check_both(got, r, g, 'enc', i, cases[i]['mask'], (cap, names[i]))
                assert (got['counts'][r, runs[r]:].view(np.uint32) == GUARD32).all(), (cap, names[i])
                assert (got['chars'][r, got['n_bytes'][r]:] == GUARD8).all(), (cap, names[i])
            else:
                assert got['n_bytes'][r] == 0, (cap, names[i])
                assert (got['chars'][r] == GUARD8).all(), (cap, names[i])       # no part of a string that does not fit


# ------------------------------------------------------------------------------------------------ mask IoU
def _iou_equal(got, o, inter, where):
    got_o, got_i = got
    assert got_o.dtype == torch.float64 and tuple(got_o.shape) == o.shape, where          # o[g * M + d]
    assert got_o.cpu().numpy().tobytes() == o.tobytes(), where
    assert np.array_equal(words(got_i), inter), where


@pytest.mark.parametrize("size", E.IOU_SIZES, ids=lambda s: "%dx%d" % s)
def test_iou_sets_clean_and_dirty_crowd_and_not(cuda, golden_dir, size):
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    h, w = size
    names, dt, gt = E.iou_masks(h, w, 900 + E.IOU_SIZES.index(size))
    key = 'iou_%dx%d' % size
    crowd = E.iou_crowd(len(gt))
    stated = {k: R.iou(dt, gt, c) for k, c in (('_o0', crowd), ('_o1', 1 - crowd))}
    for dirty in (False, True):
        d = dev_words(np.stack([E.pack(m, dirty=dirty) for m in dt]), cuda)
        t = dev_words(np.stack([E.pack(m, dirty=dirty) for m in gt]), cuda)
        for k, c in (('_o0', crowd), ('_o1', 1 - crowd)):
            got = N.mask_iou(d, t, size, dev(c, cuda))
            _iou_equal(got, g[key + k], g[key + '_inter'], (key, k, dirty, 'fixture'))
            _iou_equal(got, stated[k][0], stated[k][1], (key, k, dirty, 'statement'))
    if size == (66, 96):                                                      # M = N = 1: the full plane against the single last pixel
        d, t = names.index('full'), names.index('last')
        got = N.mask_iou(dev_words(E.pack(dt[d], dirty=True)[None], cuda), dev_words(E.pack(gt[t])[None], cuda), size,
                         dev(crowd[t:t + 1], cuda))
        _iou_equal(got, g[key + '_o0'][t:t + 1, d:d + 1], g[key + '_inter'][t:t + 1, d:d + 1], 'M = N = 1')


def test_iou_of_70_against_3(cuda, golden_dir):
    """M != N: an index taken as o[d * N + g] shows"""
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    dt, gt, crowd = E.iou_m70()
    got = N.mask_iou(dev_words(np.stack([E.pack(m) for m in dt]), cuda), dev_words(np.stack([E.pack(m) for m in gt]), cuda), (E.H, E.W),
                     dev(crowd, cuda))
    _iou_equal(got, g['iou_m70_o'], g['iou_m70_inter'], 'fixture')
    so, si = R.iou(dt, gt, crowd)
    _iou_equal(got, so, si, 'statement')
    assert tuple(got[0].shape) == (3, 70)


# ------------------------------------------------------------------------------------------------ annToMask
def _frpoly_guarded(cuda, flat, n, H, Wd, calls=1):
    """native.mask_frpoly into planes pre-filled with ones, with guard words round out, area and the workspace -> (words of every call,
    area, the device planes); the guards are asserted here"""
    from scda_amd import native as N
    P, Q = len(flat['poly_plane']), len(flat['rle_plane'])
    need = N.mask_frpoly_workspace_bytes(P, Q, H, Wd)
    wsbuf = torch.full((need + 32,), GUARD8, dtype=torch.uint8, device=cuda)
    obuf = torch.full((n * H * Wd + 8,), GUARD32, dtype=torch.int32, device=cuda)
    abuf = torch.full((n + 2,), GUARD32, dtype=torch.int32, device=cuda)
    bits, area = obuf[4:4 + n * H * Wd].view(n, H, Wd), abuf[1:1 + n]
    bits.fill_(-1)
    args = [N.upload(flat[k] if k != 'rle_counts' else flat[k].view(np.int32), cuda)
            for k in ('xy', 'poly_first', 'poly_plane', 'rle_counts', 'rle_first', 'rle_plane', 'sizes')]
    out = []
    for _ in range(calls):
        assert N.mask_frpoly(*args, wsbuf[16:16 + need], bits, area=area) is bits
        out.append(words(bits).copy())
    torch.cuda.synchronize()
    assert bool((obuf[:4] == GUARD32).all()) and bool((obuf[-4:] == GUARD32).all()), "written outside the planes"
    assert int(abuf[0]) == GUARD32 and int(abuf[-1]) == GUARD32, "written outside the areas"
    assert bool((wsbuf[:16] == GUARD8).all()) and bool((wsbuf[-16:] == GUARD8).all()), "written outside the workspace"
    return out, words(area).copy(), bits


def _through_string_decode(planes):
    """the flat arrays with the counts of every string case taken from the host's decode of its string"""
    from scda_amd import coco_gt
    planes = [c if c is None or c['string'] is None else dict(c, counts=coco_gt.counts_from_string(c['string'])) for c in planes]
    return E.flat_annotations(planes)


_RUNS = {}


def _rasterised(cuda, prefix):
    if prefix not in _RUNS:
        planes, H, Wd = (E.poly_cases(), E.H, E.WD) if prefix == 'poly' else (E.poly_big_cases(), E.BIG['H'], E.BIG['Wd'])
        _RUNS[prefix] = (planes,) + _frpoly_guarded(cuda, _through_string_decode(planes), len(planes), H, Wd, calls=2)
    return _RUNS[prefix]


@pytest.mark.parametrize("prefix", ("poly", "polybig"))
def test_planes_and_areas_equal_the_reference_and_the_statement(cuda, golden_dir, prefix):
    g = E.fixture(golden_dir)
    planes, got, area, _ = _rasterised(cuda, prefix)
    H, Wd = got[0].shape[1:]
    assert got[0].tobytes() == got[1].tobytes()                               # a second call into the same buffers: identical bytes
    bad = []
    for n, c in enumerate(planes):
        name = 'plane %d: no shape' % n if c is None else c['name']
        stated = np.zeros((H, Wd), np.uint32) if c is None else E.pack(
            mp.annotation(c['h'], c['w'], c['polygons'], None if c['counts'] is None else c['counts']), H, Wd)
        # the whole plane, every word written: the planes were all ones before the call
        if not (np.array_equal(got[0][n], g[prefix + '_bits'][n]) and np.array_equal(got[0][n], stated)):
            bad.append(name)
        if int(area[n]) != int(g[prefix + '_area'][n]):
            bad.append(name + ' (area)')
    assert not bad, bad


def test_mask_rle_gives_back_the_counts_of_rle_fr_poly(cuda, golden_dir):
    from scda_amd import native as N
    g = E.fixture(golden_dir)
    planes, _, _, bits = _rasterised(cuda, 'poly')
    single = [n for n, c in enumerate(planes) if c is not None and len(c['polygons']) == 1 and c['counts'] is None]
    assert len(single) == 8 * len(E.POLY_SIZES)
    want = [E.cut(g['poly_frpoly'], g['poly_frpoly_first'], n) for n in single]
    sizes = torch.tensor([[planes[n]['h'], planes[n]['w']] for n in single], dtype=torch.float32, device=cuda)
    got = host(N.mask_rle(bits[single].contiguous(), image_info=sizes, cap_runs=max(len(c) for c in want)))
    for r, n in enumerate(single):
        assert got['n_runs'][r] == len(want[r]) and np.array_equal(got['counts'][r, :len(want[r])].view(np.uint32), want[r]), planes[n]['name']


def test_inputs_the_reference_does_not_define(cuda):
    """include/scda_ops.h: coordinates up to +-65535 are taken; a shape whose plane index or size is out of range is skipped, as if it
    were absent; an edge with a vertex that is not finite or beyond +-65535 and the run ends behind h * w are skipped, and that plane
    is unspecified -- but it is written, zero outside its image, and nothing else changes"""
    h, w = 33, 31
    rect = np.array([[2, 3], [20, 3], [20, 30], [2, 30]], dtype=np.float64)
    far = np.array([[-65535, 10], [65535, 20], [15, 65535], [12, -65535]], dtype=np.float64)
    case = lambda polygons=(), counts=None, size=(h, w): {'h': size[0], 'w': size[1], 'polygons': list(polygons), 'counts': counts}   # noqa: E731
    beyond, nan = far.copy(), rect.copy()
    beyond[1, 0] = np.nextafter(65535.0, np.inf)
    nan[2, 1] = np.nan
    u32 = lambda *v: np.array(v, dtype=np.uint32)                             # noqa: E731
    planes = [case([rect]), case([far]), case([rect, beyond]), case(counts=u32(7, 100, 50, 3)), case([nan]), case([rect], size=(66, 96)),
              case([rect], u32(5, 9), size=(67, 96)), case(counts=u32(10, 20, 0xffffff00, 0xffffff00, 5)), case([rect], u32(0, h * w))]
    unspecified, skipped = (2, 4, 7), (6,)
    flat = E.flat_annotations(planes)
    n = len(planes)
    # shapes of plane -1 in front and of plane N behind (the plane lists stay non-decreasing)
    flat['xy'] = np.concatenate([rect, flat['xy'], rect])
    flat['poly_first'] = np.concatenate([[0], flat['poly_first'] + 4, [flat['poly_first'][-1] + 8]]).astype(np.int32)
    flat['poly_plane'] = np.concatenate([[-1], flat['poly_plane'], [n]]).astype(np.int32)
    flat['rle_counts'] = np.concatenate([u32(3, 4), flat['rle_counts'], u32(0, 9)])
    flat['rle_first'] = np.concatenate([[0], flat['rle_first'] + 2, [flat['rle_first'][-1] + 4]]).astype(np.int32)
    flat['rle_plane'] = np.concatenate([[-1], flat['rle_plane'], [n]]).astype(np.int32)
    got, area, _ = _frpoly_guarded(cuda, flat, n, E.H, E.WD, calls=2)
    assert got[0].tobytes() == got[1].tobytes()
    for i, c in enumerate(planes):
        if i in skipped:
            assert not got[0][i].any() and area[i] == 0, i                    # as if its shapes were absent
        elif i in unspecified:
            inside = E.pack(np.ones((c['h'], c['w']), bool))
            assert not (got[0][i] & ~inside).any(), i                         # written, and nothing outside the image
            assert int(area[i]) == int(R.unpack(got[0][i], c['h'], c['w']).sum()), i
        else:
            want = mp.annotation(c['h'], c['w'], c['polygons'], c['counts'])
            assert np.array_equal(got[0][i], E.pack(want)) and int(area[i]) == int(want.sum()), i
    assert area[1] > 0 and area[0] == area[5]
