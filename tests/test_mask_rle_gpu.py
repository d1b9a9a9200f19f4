"""COCO run-length results on the MI355X (scda_amd/csrc/mask_rle.hip): the encoder and the mask IoU against the reference's recorded
outputs (tests/golden/mask_rle_ref.npz) and the numpy statement (tests/mask_rle_np.py) bit for bit, pasted masks at 800 x 1344 with
and without the window hint, the capacity contract, and Predictor(masks=True, rle=True) with segm_rows, graph replay and the host
fallback."""
import numpy as np
import pytest
import torch

import mask_rle_np as R
from gpu_arrays import check_mask as _check_mask, dev as _dev, dev_words as _bits, host as _host
from test_mask_rle_rules import GROUPS, IOU_SETS, fixture_cases, iou_set

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", GROUPS)
def test_encode_equals_the_reference_and_the_statement(cuda, golden_dir, group):
    from scda_amd import native as N
    cases = fixture_cases(golden_dir, group)
    bits = np.stack([c[0] for c in cases])
    sizes = np.array([c[1] for c in cases], dtype=np.float32)
    cap = max(len(c[2]) for c in cases)
    got = _host(N.mask_rle(_bits(bits, cuda), image_info=_dev(sizes, cuda), cap_runs=cap))
    for r, (plane, (h, w), counts, chars, area, bbox) in enumerate(cases):
        _check_mask(got, r, {'n_runs': len(counts), 'counts': counts, 'chars': chars, 'area': area, 'bbox': bbox}, (group, r, 'fixture'))
        _check_mask(got, r, R.statement(R.unpack(plane, h, w)), (group, r, 'statement'))
    # one size for all masks: the convenience form (the first case's size, whatever lies outside it does not count)
    h, w = cases[0][1]
    got = _host(N.mask_rle(_bits(bits, cuda), size=(h, w), cap_runs=h * w + 1))
    for r, c in enumerate(cases):
        _check_mask(got, r, R.statement(R.unpack(c[0], h, w)), (group, r, 'one size'))


def _pasted(cuda, smooth):
    """100 packed masks at 800 x 1344 from mask_paste: seeded planes and boxes as test_paste_equals_host_predict_masks_at_800x1344 builds
    them (noise masks), or a Gaussian bump per RoI (blobs)"""
    from scda_amd import native as N
    from test_mask_infer_gpu import _mixed_rois
    H, W, n = 800, 1344, 100
    rng = np.random.RandomState(31)
    rois = _mixed_rois(rng, n, H, W)
    if smooth:
        yy, xx = np.mgrid[:28, :28].astype(np.float32)
        cy, cx = rng.uniform(9, 18, (2, n, 1, 1)).astype(np.float32)
        s = rng.uniform(4, 9, (n, 1, 1)).astype(np.float32)
        planes = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)).astype(np.float32)
    else:
        planes = rng.rand(n, 28, 28).astype(np.float32)
    rois_d = _dev(rois, cuda)
    bits = N.mask_paste(rois_d, _dev(planes, cuda), H, W, packed=True, threshold=0.5)
    return bits, rois_d, H, W


@pytest.mark.parametrize("smooth", (False, True))
def test_pasted_masks_at_800x1344(cuda, smooth):
    from scda_amd import native as N
    bits, rois, H, W = _pasted(cuda, smooth)
    words = bits.cpu().numpy().view(np.uint32)
    want = [R.statement(R.unpack(words[r], H, W)) for r in range(words.shape[0])]
    most = max(s['n_runs'] for s in want)
    print("smooth" if smooth else "noise", "runs per mask: max %d  mean %.0f  (default capacity %d)"
          % (most, np.mean([s['n_runs'] for s in want]), 4 * W))
    cap = most if not smooth else 4 * W
    plain = N.mask_rle(bits, size=(H, W), cap_runs=cap)
    got = _host(plain)
    for r, s in enumerate(want):
        _check_mask(got, r, s, (smooth, r))
    hinted = N.mask_rle(bits, size=(H, W), rois=rois, cap_runs=cap)
    again = N.mask_rle(bits, size=(H, W), cap_runs=cap)
    hp, ha = _host(hinted), _host(again)
    for r, s in enumerate(want):
        _check_mask(hp, r, s, (smooth, r, 'hint'))
        _check_mask(ha, r, s, (smooth, r, 'again'))
    for k in ('n_runs', 'n_bytes', 'area', 'bbox'):
        assert torch.equal(plain[k], hinted[k]) and torch.equal(plain[k], again[k]), k
    if smooth:
        # the condition that keeps the default capacity honest: blob masks stay under 4 * W runs, none overflows
        default = N.mask_rle(bits, size=(H, W))
        assert default['counts'].shape[1] == 4 * W
        assert int((default['n_runs'] > 4 * W).sum()) == 0 and most <= 4 * W


def test_capacity_is_exact_and_nothing_is_written_past_it(cuda, golden_dir):
    from scda_amd import native as N
    cases = fixture_cases(golden_dir, 'mid')
    bits = np.stack([c[0] for c in cases])
    sizes = np.array([c[1] for c in cases], dtype=np.float32)
    runs = np.array([len(c[2]) for c in cases])
    victim = int(np.argsort(runs)[len(runs) // 2])                         # a mask in the middle of the range
    guard = 0x5a
    for cap, flagged in ((int(runs[victim]), False), (int(runs[victim]) - 1, True)):
        n, cb = len(cases), cap * N.mask_rle_max_chars(70, 96)
        # counts and chars live inside larger buffers filled with a guard pattern: a word in front, a word behind
        cbuf = torch.full((n * cap + 2,), 0x5a5a5a5a, dtype=torch.int32, device=cuda)
        sbuf = torch.full((n * cb + 32,), guard, dtype=torch.uint8, device=cuda)
        out = {'n_runs': torch.empty(n, dtype=torch.int32, device=cuda), 'counts': cbuf[1:1 + n * cap].view(n, cap),
               'n_bytes': torch.empty(n, dtype=torch.int32, device=cuda), 'chars': sbuf[16:16 + n * cb].view(n, cb),
               'area': torch.empty(n, dtype=torch.int32, device=cuda), 'bbox': torch.empty(n, 4, dtype=torch.int32, device=cuda)}
        N.mask_rle(_bits(bits, cuda), image_info=_dev(sizes, cuda), cap_runs=cap, out=out)
        got = _host(out)
        assert int(cbuf[0]) == 0x5a5a5a5a and int(cbuf[-1]) == 0x5a5a5a5a
        assert bool((sbuf[:16] == guard).all()) and bool((sbuf[-16:] == guard).all())
        assert np.array_equal(got['n_runs'], runs)                           # the true count, also beyond the capacity
        assert (got['n_runs'][victim] > cap) == flagged
        for r, (plane, (h, w), counts, chars, area, bbox) in enumerate(cases):
            assert int(got['area'][r].view(np.uint32)) == area and got['bbox'][r].tolist() == bbox
            if runs[r] <= cap:                                                # the neighbours of an overflowing mask are untouched
                _check_mask(got, r, {'n_runs': len(counts), 'counts': counts, 'chars': chars, 'area': area, 'bbox': bbox}, (cap, r))
                assert (got['counts'][r, runs[r]:].view(np.uint32) == 0x5a5a5a5a).all()
                assert (got['chars'][r, got['n_bytes'][r]:] == guard).all()
            else:
                assert got['n_bytes'][r] == 0
                assert (got['chars'][r] == guard).all()                       # no part of a string that does not fit


@pytest.mark.parametrize("name", IOU_SETS)
def test_iou_equals_the_reference_and_the_statement(cuda, golden_dir, name):
    from scda_amd import native as N
    dt, gt, (h, w), crowd, o, inter = iou_set(golden_dir, name)
    got_o, got_i = N.mask_iou(_bits(dt, cuda), _bits(gt, cuda), (h, w), None if crowd is None else _dev(crowd, cuda))
    assert got_o.dtype == torch.float64 and tuple(got_o.shape) == (gt.shape[0], dt.shape[0])          # o[g * M + d]
    assert got_o.cpu().numpy().tobytes() == o.tobytes()
    assert np.array_equal(got_i.cpu().numpy().view(np.uint32), inter)
    so, si = R.iou(R.unpack(dt, h, w), R.unpack(gt, h, w), crowd)
    assert got_o.cpu().numpy().tobytes() == so.tobytes() and np.array_equal(got_i.cpu().numpy().view(np.uint32), si)


def test_iou_of_pasted_masks_and_packed_ground_truth(cuda):
    """masks as the detector leaves them against ground truth packed on the host, inside a crop of the padded plane"""
    from scda_amd import infer, native as N
    bits, _, H, W = _pasted(cuda, True)
    h, w = 780, 1301
    dt = bits[:12].contiguous()
    rng = np.random.RandomState(4)
    gt = np.zeros((5, H, W), dtype=bool)
    for g in range(5):
        y, x = rng.randint(0, 500), rng.randint(0, 900)
        gt[g, y:y + rng.randint(40, 300), x:x + rng.randint(40, 440)] = True
    gt[4] = R.unpack(dt[3].cpu().numpy(), H, W)                              # one identical pair (up to the crop)
    crowd = np.array([0, 1, 0, 0, 1], dtype=np.uint8)
    got_o, got_i = N.mask_iou(dt, infer.pack_masks(gt).to(cuda), (h, w), _dev(crowd, cuda))
    so, si = R.iou(R.unpack(dt.cpu().numpy(), h, w), gt[:, :h, :w], crowd)
    assert got_o.cpu().numpy().tobytes() == so.tobytes() and np.array_equal(got_i.cpu().numpy().view(np.uint32), si)
    assert so[4, 3] == 1.0 and (so > 0).sum() > 3


def _segm_statement(out, W):
    """segm_rows' expected value from the SAME pass's mask_rows output"""
    from scda_amd import infer
    size = out[5]['size'].cpu().numpy()
    want = []
    for b, masks in enumerate(infer.mask_rows(out[4], out[3], W)):
        h, w = int(size[b, 0]), int(size[b, 1])
        rows = []
        for m in masks:
            s = R.statement(m[:h, :w])
            rows.append({'size': [h, w], 'counts': s['chars'].decode('ascii'), 'area': s['area'], 'bbox': s['bbox']})
        want.append(rows)
    return want


def test_predictor_rle_equals_the_statement_on_its_own_masks(cuda):
    from scda_amd import infer
    from test_mask_infer_gpu import H_IMG, W_IMG, _images, _mask_detector
    det, cfg = _mask_detector(cuda)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.0], [H_IMG - 16, W_IMG - 40, 1.0]])              # the second image is padded in the batch
    with pytest.raises(ValueError):
        infer.Predictor(det, cfg, rle=True)
    pr = infer.Predictor(det, cfg, masks=True, rle=True)
    out = pr(x, info)
    plain = infer.Predictor(det, cfg, masks=True)(x, info)
    assert len(out) == 6 and len(plain) == 5
    for a, b in zip(out[:5], plain):
        assert torch.equal(a, b)
    rle = out[5]
    top_n = out[2].shape[1]
    assert tuple(rle['counts'].shape) == (2, top_n, 4 * W_IMG) and rle['size'].cpu().tolist() == [[H_IMG, W_IMG], [H_IMG - 16, W_IMG - 40]]
    counts = out[3].cpu().numpy()
    assert counts.min() > 0
    want = _segm_statement(out, W_IMG)
    rows, n_fb = infer.segm_rows(out, with_fallbacks=True)
    assert rows == want
    assert n_fb == int((rle['n_runs'] > 4 * W_IMG).sum())
    # padding detections carry the empty-mask code
    pad = torch.zeros_like(out[3])
    padded = (out[0], out[1], out[2], pad + top_n, out[4], out[5])
    for b, rows_b in enumerate(infer.segm_rows(padded)):
        h, w = rle['size'][b].tolist()
        for j in range(int(counts[b]), top_n):
            assert rows_b[j] == {'size': [h, w], 'counts': R.to_string([h * w]).decode('ascii'), 'area': 0, 'bbox': [0, 0, 0, 0]}
            assert int(rle['n_runs'][b, j]) == 1
    # a deliberately small capacity: masks overflow, the host encodes them, the results do not change
    small = infer.Predictor(det, cfg, masks=True, rle=True, rle_capacity=24)
    out_s = small(x, info)
    assert torch.equal(out_s[4], out[4])
    rows_s, n_fb_s = infer.segm_rows(out_s, with_fallbacks=True)
    assert n_fb_s > 0 and rows_s == want
    # infer.predict passes the arguments through
    again = infer.predict(det, x, info, cfg, masks=True, rle=True)
    assert len(again) == 6 and infer.segm_rows(again) == want


def test_predictor_rle_replays_as_graph(cuda):
    from scda_amd import infer
    from test_mask_infer_gpu import H_IMG, W_IMG, _images, _mask_detector
    det, cfg = _mask_detector(cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.0], [H_IMG - 7, W_IMG - 33, 1.0]], device=cuda)
    sets = [_images(s, 2, cuda) for s in (81, 82)]
    pred = infer.Predictor(det, cfg, masks=True, rle=True)
    want = []
    for y in sets:
        o = pred(y, info)
        want.append(([t.clone() for t in o[:5]], {k: v.clone() for k, v in o[5].items()}, infer.segm_rows(o)))
    assert want[0][2] != want[1][2]
    pred.capture(_images(84, 2, cuda), info)
    for y, (tensors, rle, rows) in zip(sets, want):
        pred.images.copy_(y)
        got = pred.replay()
        torch.cuda.synchronize()
        assert len(got) == 6
        for a, b in zip(got[:5], tensors):
            assert torch.equal(a, b)
        for k in ('n_runs', 'n_bytes', 'area', 'bbox', 'size'):
            assert torch.equal(got[5][k], rle[k]), k
        assert infer.segm_rows(got) == rows == _segm_statement(got, W_IMG)
