"""evaluate.write_segm_results on a pass that carries original-size results (infer.OriginalSizeResult), from a recorded pass on the
host: the line layout of the reference's result file for resize_scale != 1 -- the box divided by the scale, the
segmentation at [origin_h, origin_w] --, the ValueError of a pass without original_size unchanged, a flagged image refused.  CPU only."""
import io
import json

import numpy as np
import pytest
import torch

import mask_rle_np as RLE


def _recorded_pass(cap=100):
    """B = 2, top_n = 4 with 3 and 2 real detections, original sizes (9, 14) and (6, 40) in planes of (10, 40); the run-length results
    as the device leaves them (the third mask of image 0 has more runs than the capacity: n_bytes 0, encoded by the host from
    mask_bits_orig)"""
    from scda_amd import infer
    rng = np.random.RandomState(2)
    B, top_n, Ho, Wo = 2, 4, 10, 40
    sizes = [(9, 14), (6, 40)]
    scales = [1.6, 0.5]
    counts = [3, 2]
    det = np.zeros((B, top_n, 7), dtype=np.float32)
    masks = np.zeros((B, top_n, Ho, Wo), dtype=bool)
    for b in range(B):
        oh, ow = sizes[b]
        for j in range(counts[b]):
            x1, y1 = rng.rand(2) * 10
            det[b, j] = (b, x1, y1, x1 + 3 + rng.rand() * 9, y1 + 2 + rng.rand() * 5, np.round(rng.rand(), 3), 1 + rng.randint(5))
            masks[b, j, 1 + j:oh - 1, 2:ow - 3 - j] = True
    det[0, :3, 5] = (0.9, 0.9, 0.95)                              # the third ranks first; equal scores keep the detections' order
    masks[0, 2, :9, :14] = (np.add.outer(np.arange(9), np.arange(14)) % 2).astype(bool)      # a checkerboard: 126 runs
    rle = {'n_runs': np.zeros((B, top_n), np.int32), 'counts': np.zeros((B, top_n, cap), np.int32), 'n_bytes': np.zeros((B, top_n), np.int32),
           'chars': np.zeros((B, top_n, cap * 2), np.uint8), 'area': np.zeros((B, top_n), np.int32), 'bbox': np.zeros((B, top_n, 4), np.int32),
           'size': np.array(sizes, dtype=np.int32)}
    strings = [[] for _ in range(B)]
    for b in range(B):
        oh, ow = sizes[b]
        for j in range(top_n):
            st = RLE.statement(masks[b, j, :oh, :ow])
            if j < counts[b]:
                strings[b].append(st['chars'].decode('ascii'))
            rle['n_runs'][b, j], rle['area'][b, j], rle['bbox'][b, j] = st['n_runs'], st['area'], st['bbox']
            if st['n_runs'] <= cap:
                rle['n_bytes'][b, j] = len(st['chars'])
                rle['chars'][b, j, :len(st['chars'])] = np.frombuffer(st['chars'], np.uint8)
    assert rle['n_runs'][0, 2] > cap
    det_orig = det.copy()
    det_orig[:, :, 1:5] = det[:, :, 1:5] / np.array(scales, dtype=np.float32).reshape(B, 1, 1)
    t = torch.from_numpy
    entries = (None, None, t(det), torch.tensor(counts, dtype=torch.int32), torch.zeros(B, top_n, 16, 1, dtype=torch.int32),
               {k: t(v) for k, v in rle.items()}, infer.pack_masks(masks.reshape(B * top_n, Ho, Wo)).reshape(B, top_n, Ho, 2), t(det_orig),
               torch.zeros(B, dtype=torch.int32))
    out = infer.OriginalSizeResult(entries, {'mask_bits_orig': 6, 'det_orig': 7, 'orig_status': 8, 'rle': 5})
    info = np.array([[16, 22, scales[0], 9, 14], [3, 20, scales[1], 6, 40]], dtype=np.float32)
    return out, info, det, counts, strings


def test_lines_carry_the_original_size_results_field_by_field():
    """one JSON object per line; per image the detections by descending score, equal scores in the detections' order; the keys in the
    order image_id, bbox, score, category_id, segmentation; bbox = (x, y, w, h) of the float32 box / float32 scale; segmentation =
    {'size': [origin_h, origin_w], 'counts': the mask's string}"""
    from scda_amd import evaluate
    out, info, det, counts, strings = _recorded_pass()
    writer = io.StringIO()
    fallbacks = evaluate.write_segm_results(writer, info, [139, 285], out)
    assert fallbacks == 1                                         # the checkerboard, encoded from mask_bits_orig
    text = writer.getvalue()
    assert text.endswith('\n') and text.count('\n') == 5
    rows = [json.loads(x) for x in text.splitlines()]
    expected = [(0, 2), (0, 0), (0, 1), (1, 0), (1, 1)] if det[1, 0, 5] >= det[1, 1, 5] else [(0, 2), (0, 0), (0, 1), (1, 1), (1, 0)]
    for row, (b, j) in zip(rows, expected):
        assert list(row) == ['image_id', 'bbox', 'score', 'category_id', 'segmentation']
        assert row['image_id'] == [139, 285][b] and row['category_id'] == int(det[b, j, 6]) and row['score'] == float(det[b, j, 5])
        x1, y1, x2, y2 = (det[b, j, 1:5] / info[b, 2]).astype(np.float32)          # float32 / float32
        assert row['bbox'] == [float(x1), float(y1), float(x2) - float(x1), float(y2) - float(y1)]   # w, h: differences in double
        assert row['bbox'][0] != float(det[b, j, 1])                               # the scale was applied
        assert row['segmentation'] == {'size': [int(info[b, 3]), int(info[b, 4])], 'counts': strings[b][j]}
        assert list(row['segmentation']) == ['size', 'counts']
    # keep_num and category_of pass through
    writer = io.StringIO()
    evaluate.write_segm_results(writer, info, [139, 285], out, category_of=lambda c: 10 * c, keep_num=1)
    rows = [json.loads(x) for x in writer.getvalue().splitlines()]
    assert len(rows) == 2 and rows[0]['category_id'] == 10 * int(det[0, 2, 6]) and rows[0]['score'] == float(det[0, 2, 5])


def test_pass_without_original_size_still_raises():
    from scda_amd import evaluate
    out, info, _, _, _ = _recorded_pass()
    with pytest.raises(ValueError, match="resize_scale != 1"):
        evaluate.write_segm_results(io.StringIO(), info, [139, 285], tuple(out[:6]))
    with pytest.raises(ValueError):
        evaluate.write_segm_results(io.StringIO(), info, [139, 285], out, input_resolution=True)


def test_flagged_image_is_refused():
    from scda_amd import evaluate, infer
    out, info, _, _, _ = _recorded_pass()
    flagged = infer.OriginalSizeResult(tuple(out[:8]) + (torch.tensor([0, 4], dtype=torch.int32),), out._names)
    with pytest.raises(ValueError, match="status"):
        evaluate.write_segm_results(io.StringIO(), info, [139, 285], flagged)
