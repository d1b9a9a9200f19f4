"""The rules of the device run-length encoder and mask IoU (include/scda_ops.h), without a GPU: the numpy statement of
tests/mask_rle_np.py and the product's host fallback encoder (scda_amd/mask_rle_host.py) equal every recorded output of the reference's
compiled maskApi.c (tests/golden/mask_rle_ref.npz, tests/golden/make_golden_mask_rle.py) bit for bit; pack_masks inverts mask_rows'
unpacking; write_segm_results writes the reference's keys and refuses resize_scale != 1."""
import io
import json
import os

import numpy as np
import pytest
import torch

import mask_rle_np as R

GROUPS = ('small', 'mid', 'big')
IOU_SETS = ('wrap', 'wrap_crowd', 'mid', 'mid_crowd', 'big', 'big_crowd')


def fixture_cases(golden_dir, group):
    """-> list of (bits uint32 [H, Wd], (h, w), counts, chars bytes, area, bbox [4]) as the reference recorded them"""
    g = np.load(os.path.join(golden_dir, "mask_rle_ref.npz"))
    n_runs, n_bytes = g[group + '_n_runs'], g[group + '_n_bytes']
    co, bo = np.concatenate([[0], np.cumsum(n_runs)]), np.concatenate([[0], np.cumsum(n_bytes)])
    out = []
    for i in range(len(n_runs)):
        out.append((g[group + '_bits'][i], tuple(int(v) for v in g[group + '_sizes'][i]), g[group + '_counts'][co[i]:co[i + 1]],
                    g[group + '_chars'][bo[i]:bo[i + 1]].tobytes(), int(g[group + '_area'][i]),
                    [int(v) for v in g[group + '_bbox'][i]]))
    return out


def iou_set(golden_dir, name):
    """-> (dt bits [M, H, Wd], gt bits [N, H, Wd], (h, w), iscrowd uint8 [N] or None, o [N, M], inter [N, M])"""
    g = np.load(os.path.join(golden_dir, "mask_rle_ref.npz"))
    grp = str(g['iou_%s_group' % name])
    di, gi = g['iou_%s_dt' % name], g['iou_%s_gt' % name]
    crowd = g['iou_%s_iscrowd' % name]
    size = tuple(int(v) for v in g[grp + '_sizes'][di[0]])
    return (g[grp + '_bits'][di], g[grp + '_bits'][gi], size, crowd if crowd.size else None, g['iou_%s_o' % name],
            g['iou_%s_inter' % name])


def test_fixture_holds_the_cases_the_rules_name(golden_dir):
    small = fixture_cases(golden_dir, 'small')
    assert small[0][2].tolist() == [60] and small[0][5] == [0, 0, 0, 0]                   # empty: the single run h * w
    assert small[1][2].tolist() == [0, 60]                                                # full: the first run is 0
    assert small[8][5] == [1, 3, 2, 3]                                                    # the wrapped run: end points' rows only
    dt, gt, size, crowd, o, inter = iou_set(golden_dir, 'wrap')
    assert o[0, 0] == 0.0 and inter[0, 0] == 2 and o[1, 0] == 1.0                         # gated although 2 pixels intersect
    lengths = set()
    for _, _, counts, chars, _, _ in fixture_cases(golden_dir, 'big'):
        x = counts.astype(np.int64)
        x[3:] -= counts[1:-2].astype(np.int64)
        for v in x:
            lengths.add((len(R.to_string(np.array([v]))), bool(v < 0)))
    assert {(n, False) for n in range(1, 6)} <= lengths and {(n, True) for n in range(1, 6)} <= lengths
    assert os.path.getsize(os.path.join(golden_dir, "mask_rle_ref.npz")) <= os.path.getsize(
        os.path.join(golden_dir, "predict_masks_sweep.npz"))


@pytest.mark.parametrize("group", GROUPS)
def test_numpy_statement_equals_the_reference(golden_dir, group):
    for i, (bits, (h, w), counts, chars, area, bbox) in enumerate(fixture_cases(golden_dir, group)):
        s = R.statement(R.unpack(bits, h, w))
        assert s['n_runs'] == len(counts) and np.array_equal(s['counts'], counts), (group, i)
        assert s['chars'] == chars, (group, i)
        assert s['area'] == area and s['bbox'] == bbox, (group, i, s['bbox'], bbox)


@pytest.mark.parametrize("group", GROUPS)
def test_host_fallback_encoder_equals_the_reference(golden_dir, group):
    from scda_amd import mask_rle_host as host
    for i, (bits, (h, w), counts, chars, area, bbox) in enumerate(fixture_cases(golden_dir, group)):
        m = R.unpack(bits, h, w)
        assert np.array_equal(host.rle_counts(m), counts), (group, i)
        e = host.encode(m)
        assert e == {'size': [h, w], 'counts': chars.decode('ascii'), 'area': area, 'bbox': bbox}, (group, i)


@pytest.mark.parametrize("name", IOU_SETS)
def test_numpy_iou_equals_the_reference(golden_dir, name):
    dt, gt, (h, w), crowd, o, inter = iou_set(golden_dir, name)
    got_o, got_i = R.iou(R.unpack(dt, h, w), R.unpack(gt, h, w), crowd)
    assert got_o.tobytes() == o.tobytes() and np.array_equal(got_i, inter)


def test_pack_masks_inverts_mask_rows():
    from scda_amd import infer
    rng = np.random.RandomState(5)
    for (n, H, W) in ((3, 9, 70), (2, 5, 64), (1, 1, 1), (4, 33, 31)):
        m = rng.rand(n, H, W) < 0.4
        words = infer.pack_masks(m)
        assert words.dtype == torch.int32 and tuple(words.shape) == (n, H, (W + 31) // 32)
        back = infer.mask_rows(words[None], torch.tensor([n], dtype=torch.int32), width=W)
        assert len(back) == 1 and np.array_equal(back[0], m)
        c = (W - 1)
        assert bool((int(words[0, 0, c // 32]) >> (c % 32)) & 1) == bool(m[0, 0, c])
    with pytest.raises(ValueError):
        infer.pack_masks(np.zeros((4, 4), dtype=bool))


def _fake_pass(rng, H, W, cap):
    """the result tuple of a Predictor(masks=True, rle=True) pass, made on the host: B = 2, top_n = 4, the counts 3 and 1; one mask
    flagged as overflowing, so that segm_rows has to take its plane"""
    from scda_amd import infer
    B, top_n = 2, 4
    det = np.zeros((B, top_n, 7), dtype=np.float32)
    det_counts = np.array([3, 1], dtype=np.int32)
    sizes = np.array([[H, W], [H - 3, W - 5]], dtype=np.int32)
    masks = np.zeros((B, top_n, H, W), dtype=bool)
    cb = 5 * cap
    rle = {'n_runs': np.ones((B, top_n), np.int32), 'counts': np.zeros((B, top_n, cap), np.int32),
           'n_bytes': np.zeros((B, top_n), np.int32), 'chars': np.zeros((B, top_n, cb), np.uint8), 'area': np.zeros((B, top_n), np.int32),
           'bbox': np.zeros((B, top_n, 4), np.int32), 'size': sizes}
    want = [[], []]
    for b in range(B):
        for j in range(det_counts[b]):
            x1, y1 = rng.randint(0, W - 12), rng.randint(0, H - 12)
            det[b, j] = [b, x1, y1, x1 + 10.5, y1 + 8.25, rng.rand(), rng.randint(1, 9)]
            masks[b, j, y1:y1 + 9, x1:x1 + 11] = rng.rand(9, 11) < 0.8
            h, w = sizes[b]
            s = R.statement(masks[b, j, :h, :w])
            want[b].append({'size': [int(h), int(w)], 'counts': s['chars'].decode('ascii'), 'area': s['area'], 'bbox': s['bbox']})
            rle['n_runs'][b, j] = s['n_runs']
            if s['n_runs'] <= cap:
                rle['counts'][b, j, :s['n_runs']] = s['counts']
                rle['n_bytes'][b, j] = len(s['chars'])
                rle['chars'][b, j, :len(s['chars'])] = np.frombuffer(s['chars'], dtype=np.uint8)
            rle['area'][b, j] = s['area']
            rle['bbox'][b, j] = s['bbox']
    bits = infer.pack_masks(masks.reshape(B * top_n, H, W)).view(B, top_n, H, -1)
    out = (None, None, torch.from_numpy(det), torch.from_numpy(det_counts), bits, {k: torch.from_numpy(v) for k, v in rle.items()})
    return out, want, int((rle['n_runs'] > cap).sum())


def test_segm_rows_and_the_overflow_fallback_on_host_tensors():
    from scda_amd import infer
    rng = np.random.RandomState(9)
    out, want, _ = _fake_pass(rng, 40, 70, cap=4096)
    rows, n_fb = infer.segm_rows(out, with_fallbacks=True)
    assert rows == want and n_fb == 0
    out, want, over = _fake_pass(np.random.RandomState(9), 40, 70, cap=20)            # the same masks, a capacity most of them exceed
    assert over > 0
    rows, n_fb = infer.segm_rows(out, with_fallbacks=True)
    assert rows == want and n_fb == over
    assert infer.segm_rows(out) == want


def test_write_segm_results_writes_the_reference_keys_and_refuses_a_resize():
    from scda_amd import evaluate
    out, want, _ = _fake_pass(np.random.RandomState(13), 40, 70, cap=4096)
    info = np.array([[40, 70, 1.0], [37, 65, 1.0]], dtype=np.float32)
    buf = io.StringIO()
    assert evaluate.write_segm_results(buf, info, [17, 42], out, category_of=lambda c: c + 100) == 0
    lines = [json.loads(s) for s in buf.getvalue().splitlines()]
    det, counts = out[2].numpy(), out[3].numpy()
    assert len(lines) == counts.sum()
    k = 0
    for b, img in enumerate((17, 42)):
        order = sorted(range(counts[b]), key=lambda ix: det[b, ix, 5], reverse=True)       # as the reference sorts
        for ix in order:
            res = lines[k]; k += 1
            assert set(res) == {'image_id', 'bbox', 'score', 'category_id', 'segmentation'}
            box = det[b, ix, 1:5].tolist()
            assert res['image_id'] == img and res['bbox'] == [box[0], box[1], box[2] - box[0], box[3] - box[1]]
            assert res['score'] == det[b, ix, 5].tolist() and res['category_id'] == int(det[b, ix, 6]) + 100
            assert res['segmentation'] == {'size': want[b][ix]['size'], 'counts': want[b][ix]['counts']}
            assert isinstance(res['segmentation']['counts'], str)
    scaled = info.copy(); scaled[1, 2] = 0.5
    with pytest.raises(ValueError):
        evaluate.write_segm_results(io.StringIO(), scaled, [17, 42], out)
    buf2 = io.StringIO()
    evaluate.write_segm_results(buf2, scaled, [17, 42], out, input_resolution=True, category_of=lambda c: c + 100)
    assert buf2.getvalue() == buf.getvalue()                                               # box and mask at the input resolution
    buf3 = io.StringIO()
    evaluate.write_segm_results(buf3, info, [17, 42], out, keep_num=2)
    assert len(buf3.getvalue().splitlines()) == 3


def test_native_has_no_host_path_for_the_new_operators():
    from scda_amd import native
    words = torch.zeros(2, 8, 1, dtype=torch.int32)
    with pytest.raises(native.ScdaNativeError):
        native.mask_rle(words)
    with pytest.raises(native.ScdaNativeError):
        native.mask_iou(words, words, (8, 32))
    assert native.mask_rle_max_chars(800, 1344) == 5 and native.mask_rle_max_chars(4096, 4096) == 6
    assert native.mask_rle_max_chars(1, 1) == 1 and native.mask_rle_max_chars(10, 6) == 2
