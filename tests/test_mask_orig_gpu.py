"""Segmentation results at the original image size on the MI355X (scda_amd/csrc/mask_rescale.hip, infer.Predictor(original_size=...),
evaluate.coco_stats): the fused paste-and-resize kernel bit for bit against tests/golden/segm_orig_ref.npz (the reference's predict_masks
and lines 422-423 of its write_results_to_file under Pillow), against the numpy statement tests/mask_orig_np.py and against PIL at the
workload's geometry; the limits it flags; the whole pass against the host composition from its own planes; graph replay; the COCO
stats at original coordinates against the route where the test resizes and encodes on the host.

The fixture's (1, 1) case is a 96x and 160x down-scale: the rule holds for it on the host (tests/test_mask_orig_rules.py), the kernel
flags it (status 4, a down-scale above 4) and gives empty masks -- that is what is asserted for it here."""
import copy
import os

import numpy as np
import pytest
import torch

import coco_eval_np as cnp
import mask_orig_np as O
import mask_rle_np as RLE
from gpu_arrays import dev as _dev, words as _words
from test_mask_infer_rules import own_planes, paste_statement

pytestmark = pytest.mark.gpu

H, W = 96, 160
N_CASES = 8


@pytest.fixture(scope="module")
def sweep(golden_dir):
    """the 8 cases of the fixture as ONE batch of 8 images x 24 RoIs in planes of (137, 229), with the numpy statement's results --
    computed once, left unchanged"""
    g = np.load(os.path.join(golden_dir, "segm_orig_ref.npz"))
    rois, planes = g["rois"], own_planes(g["heatmap"], g["rois"])
    sizes = [tuple(int(v) for v in g["sizes_%d" % k]) for k in range(N_CASES)]
    info = np.array([[h, w, 1.0, oh, ow] for h, w, oh, ow in sizes], dtype=np.float32)
    all_rois = np.concatenate([rois[:, :5]] * N_CASES)
    all_planes = np.concatenate([planes] * N_CASES)
    Ho, Wo = 137, 229
    want, foot, status = O.statement(all_rois, all_planes, H, W, info, 24, Ho, Wo)
    return {'gold': g, 'sizes': sizes, 'info': info, 'rois': all_rois, 'planes': all_planes, 'Ho': Ho, 'Wo': Wo, 'want': want,
            'foot': foot, 'status': status}


def _run(s, cuda, packed, threshold=0.5, cls=None):
    from scda_amd import native as N
    R = s['rois'].shape[0]
    shape = (R, s['Ho'], (s['Wo'] + 31) // 32) if packed else (R, s['Ho'], s['Wo'])
    out = torch.full(shape, 0x5a5a5a5a if packed else 777.0, dtype=torch.int32 if packed else torch.float32, device=cuda)
    foot = torch.full((R, 5), -7.0, device=cuda)
    status = torch.full((s['info'].shape[0],), -7, dtype=torch.int32, device=cuda)
    N.mask_rescale(_dev(s['rois'], cuda), _dev(s['planes'], cuda), s.get('H', H), s.get('W', W), _dev(s['info'], cuda), s['Ho'], s['Wo'],
                   cls=None if cls is None else _dev(cls, cuda), packed=packed, threshold=threshold, out=out, foot_rois=foot, status=status)
    return out, foot.cpu().numpy(), status.cpu().numpy()


def test_float_form_equals_fixture_and_statement(cuda, sweep):
    out, foot, status = _run(sweep, cuda, packed=False)
    got = out.cpu().numpy()
    assert np.array_equal(status, sweep['status']) and list(status) == [0, 0, 0, 0, 0, 0, O.FLAG_RATIO, 0]
    assert np.array_equal(foot, sweep['foot'].astype(np.float32))
    assert got.tobytes() == sweep['want'].tobytes()              # every element written (the sentinel is gone), no negative zero
    g = sweep['gold']
    for k, (h, w, oh, ow) in enumerate(sweep['sizes']):
        rows = got[k * 24:(k + 1) * 24]
        assert not rows[:, oh:].any() and not rows[:, :, ow:].any()
        if k == 6:
            assert not rows.any()                                 # the flagged (1, 1) image: empty
            continue
        for i, r in enumerate(g["rois_%d" % k]):
            assert np.array_equal(rows[r, :oh, :ow], g["orig_%d" % k][i]), (k, r)


@pytest.mark.parametrize("threshold", [0.5, 0.0, -0.1])
def test_packed_form_equals_fixture_and_statement(cuda, sweep, threshold):
    out, foot, status = _run(sweep, cuda, packed=True, threshold=threshold)
    got = _words(out)
    sizes = [(oh, ow) if st == 0 else (0, 0) for (_, _, oh, ow), st in zip(sweep['sizes'], sweep['status']) for _ in range(24)]
    assert np.array_equal(got, O.pack_gt(sweep['want'], threshold, sizes))
    assert np.array_equal(status, sweep['status']) and np.array_equal(foot, sweep['foot'].astype(np.float32))
    assert not got[6 * 24:7 * 24].any()                           # the flagged image stays empty below a negative threshold too
    if threshold == 0.5:                                          # the reference's own strings
        g = sweep['gold']
        for k, (h, w, oh, ow) in enumerate(sweep['sizes']):
            if k == 6:
                continue
            strings = g["rle_%d" % k].tobytes().split(b"\n")
            for i, r in enumerate(g["rois_%d" % k]):
                assert RLE.to_string(RLE.encode(RLE.unpack(got[k * 24 + r], oh, ow))) == strings[i], (k, r)


def test_exact_capacity_and_rle_with_the_footprint_hint(cuda, sweep):
    """planes of exactly (oh, ow) = (60, 100); scda_mask_rle_hip on them with foot_rois as its hint and image_info + 3 as its sizes"""
    from scda_amd import native as N
    g = sweep['gold']
    s = {'rois': sweep['rois'][:24], 'planes': sweep['planes'][:24], 'info': sweep['info'][:1], 'Ho': 60, 'Wo': 100}
    out, foot, status = _run(s, cuda, packed=True)
    assert status[0] == 0 and np.array_equal(_words(out), O.pack_gt(sweep['want'][:24, :60, :100], 0.5, [(60, 100)] * 24))
    rle = N.mask_rle(out, image_info=_dev(s['info'], cuda), info_column=3, rois=_dev(foot, cuda), cap_runs=60 * 100 + 1)
    strings = g["rle_0"].tobytes().split(b"\n")
    chars, n_bytes = rle['chars'].cpu().numpy(), rle['n_bytes'].cpu().numpy()
    for r in range(24):
        assert chars[r, :n_bytes[r]].tobytes() == strings[r], r


def test_padding_rows_and_flagged_images(cuda, sweep):
    """cls < 0 gives an empty mask; oh > Ho, a ratio above the limit and oh = 0 are flagged, their masks empty, the others unaffected"""
    rng = np.random.RandomState(5)
    rois = np.array([[0, 10, 20, 90, 70], [0, 0, 0, 159, 95], [0, 100, 5, 140, 60]] * 4, dtype=np.float32)
    planes = rng.rand(12, 28, 28).astype(np.float32)
    cls = np.array([1, -1, 2] + [1] * 9, dtype=np.int32)
    info = np.array([[96, 160, 1.6, 60, 100], [96, 160, 1.0, 65, 100], [96, 160, 4.2, 23, 40], [96, 160, 1.0, 0, 100]], dtype=np.float32)
    s = {'rois': rois, 'planes': planes, 'info': info, 'Ho': 64, 'Wo': 128}
    want, wfoot, wstatus = O.statement(rois, planes, H, W, info, 3, 64, 128, cls=cls)
    assert list(wstatus) == [0, O.FLAG_CAPACITY, O.FLAG_RATIO, O.FLAG_EMPTY | O.FLAG_RATIO]
    for threshold in (0.5, -0.1):
        out, foot, status = _run(s, cuda, packed=True, threshold=threshold, cls=cls)
        got = _words(out)
        assert np.array_equal(status, wstatus) and np.array_equal(foot, wfoot.astype(np.float32))
        assert np.array_equal(got, O.pack_gt(want, threshold, [(60, 100)] * 3 + [(0, 0)] * 9))
        assert not got[3:].any() and got[0].any() and got[2].any()
        assert got[1].any() == (threshold < 0)                   # the padding row: an empty mask, its bits (0.0f > threshold)
    out, foot, status = _run(s, cuda, packed=False, cls=cls)
    assert out.cpu().numpy().tobytes() == want.tobytes() and not want[1].any()


def test_workload_geometry_equals_pil(cuda):
    """padded 800 x 1344, (h, w) = (800, 1067), (oh, ow) = (480, 640): a workgroup owns 32 output columns and walks blocks of 4 output
    rows.  The whole image, a 1 x 1 box, boxes whose footprints straddle strip boundaries (output columns 32 k) and row-block
    boundaries (output rows 4 k), a box that ends on the last output column and row, a box that leaves the 1067 columns"""
    from PIL import Image
    Hp, Wp, h, w, oh, ow = 800, 1344, 800, 1067, 480, 640
    rng = np.random.RandomState(17)
    sx, sy = w / ow, h / oh
    rois = np.array([[0, 0, 0, 1066, 799],
                     [0, 533, 400, 533, 400],
                     [0, int(31.5 * sx), int(3.5 * sy), int(32.5 * sx), int(4.5 * sy)],          # around output column 32 / row 4
                     [0, int(60 * sx), int(100 * sy), int(196 * sx), int(103 * sy)],             # strips 1..6, inside one row block
                     [0, int(318 * sx), int(10 * sy), int(321 * sx), int(470 * sy)],             # around column 320, most row blocks
                     [0, 900, 700, 1066, 799],                                                   # the last column and row
                     [0, 1000, 300, 1300, 420],                                                  # leaves the image's 1067 columns
                     [0, 0.7, 0.9, 40.2, 27.9]], dtype=np.float32)
    planes = rng.rand(8, 28, 28).astype(np.float32)
    info = np.array([[h, w, 1.25, oh, ow]], dtype=np.float32)
    P = paste_statement(rois, planes, Hp, Wp)[:, :h, :w]
    want = np.stack([np.array(Image.fromarray(np.ascontiguousarray(p)).resize((ow, oh))) for p in P])
    s = {'rois': rois, 'planes': planes, 'info': info, 'Ho': oh, 'Wo': ow, 'H': Hp, 'W': Wp}
    out, foot, status = _run(s, cuda, packed=False)
    got = out.cpu().numpy()
    assert status[0] == 0
    for r in range(8):
        assert np.array_equal(got[r], want[r]), (r, np.abs(got[r] - want[r]).max())
        assert tuple(foot[r, 1:]) == O.footprint(rois[r], h, w, oh, ow), r
        inside = np.zeros((oh, ow), dtype=bool)
        inside[int(foot[r, 2]):int(foot[r, 4]) + 1, int(foot[r, 1]):int(foot[r, 3]) + 1] = True
        assert not want[r][~inside].any() and want[r].any()
    out, _, _ = _run(s, cuda, packed=True)
    assert np.array_equal(_words(out), O.pack_gt(want, 0.5, [(oh, ow)] * 8))


def test_bad_arguments(cuda):
    from scda_amd import native as N
    rois, planes = torch.zeros(4, 5, device=cuda), torch.zeros(4, 28, 28, device=cuda)
    info = torch.tensor([[96, 160, 1.0, 60, 100]] * 2, device=cuda)
    assert N.mask_rescale_max_ratio() == O.MAX_RATIO
    with pytest.raises(ValueError):
        N.mask_rescale(rois, planes, 96, 160, info[:, :4].contiguous(), 60, 100)          # no original size in the rows
    with pytest.raises(ValueError):
        N.mask_rescale(rois, planes, 96, 160, info.repeat(2, 1)[:3].contiguous(), 60, 100)   # R is no multiple of B
    with pytest.raises(ValueError):
        N.mask_rescale(rois, torch.zeros(4, 33, 28, device=cuda), 96, 160, info, 60, 100)
    with pytest.raises(ValueError):
        N.mask_rescale(rois, planes, 96, 160, info, 60, 100, packed=True, out=torch.zeros(4, 60, 3, dtype=torch.int32, device=cuda))
    with pytest.raises(N.ScdaNativeError):
        N.mask_rescale(rois, planes, 96, 160, info.cpu(), 60, 100)


# ---------------------------------------------------------------------------------------------------------------------------------
TOP_N = 16
RLE_CAP = 40000         # runs kept per mask: the untrained head's speckled masks exceed the default of 4 * Wo


def _detector(cuda):
    from test_mask_infer_gpu import _mask_detector
    det, cfg = _mask_detector(cuda)
    cfg = copy.deepcopy(cfg)
    cfg['test_predict_bbox_cfg']['top_n'] = TOP_N               # the host composition below restates every detection
    return det, cfg


@pytest.fixture(scope="module")
def whole_pass(cuda):
    """one seeded mask-branch detector, B = 2: image 0 (256 x 400) up to (320, 500), image 1 (240 x 384 inside the padded plane) down to
    (150, 240); the pass with original_size, its clones, and the host composition from the pass's OWN planes and RoIs"""
    from scda_amd import infer
    from test_mask_infer_gpu import H_IMG, W_IMG, _images
    det, cfg = _detector(cuda)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 0.8, 320, 500], [240, 384, 1.6, 150, 240]], dtype=torch.float32)
    pred = infer.Predictor(det, cfg, masks=True, rle=True, original_size=(320, 512), rle_capacity=RLE_CAP)
    res = pred(x, info)
    out = [t.clone() if torch.is_tensor(t) else {k: v.clone() for k, v in t.items()} for t in res]
    names = {k: out[res._names[k]] for k in ('mask_bits_orig', 'det_orig', 'orig_status')}
    want, foot, status = O.statement(pred.mask_rois.cpu().numpy(), pred.mask_planes.cpu().numpy(), H_IMG, W_IMG, info.numpy(), TOP_N,
                                     320, 512, cls=pred.mask_cls.cpu().numpy())
    return {'det': det, 'cfg': cfg, 'x': x, 'info': info, 'pred': pred, 'res_type': type(res), 'len': len(res), 'out': out,
            'names': names, 'want': want, 'segm': infer.segm_rows(res, with_fallbacks=True)}


def test_pass_equals_host_composition(cuda, whole_pass):
    from scda_amd import infer
    p = whole_pass
    out, info = p['out'], p['info'].numpy()
    assert p['res_type'] is infer.OriginalSizeResult and p['len'] == 9
    bits, det_orig, status = p['names']['mask_bits_orig'], p['names']['det_orig'], p['names']['orig_status']
    assert out[6] is bits and out[7] is det_orig and out[8] is status
    assert tuple(bits.shape) == (2, TOP_N, 320, 16) and bits.dtype == torch.int32 and not status.any()
    counts = out[3].cpu().numpy()
    assert counts.min() > 0
    sizes = [(320, 500)] * TOP_N + [(150, 240)] * TOP_N
    want_bits = O.pack_gt(p['want'], 0.5, sizes).reshape(2, TOP_N, 320, 16)
    assert np.array_equal(_words(bits), want_bits)
    det = out[2].cpu().numpy()
    want_det = det.copy()
    want_det[:, :, 1:5] = det[:, :, 1:5] / info[:, 2].reshape(2, 1, 1)
    assert want_det.dtype == np.float32 and det_orig.cpu().numpy().tobytes() == want_det.tobytes()
    # the run-length results: entry 5 is the ORIGINAL-size code
    rle = out[5]
    assert np.array_equal(rle['size'].cpu().numpy(), [[320, 500], [150, 240]])
    rows, fallbacks = p['segm']
    assert fallbacks == 0
    area = rle['area'].cpu().numpy()
    some = False
    for b in range(2):
        oh, ow = sizes[b * TOP_N]
        assert len(rows[b]) == counts[b]
        for j in range(int(counts[b])):
            m = p['want'][b * TOP_N + j, :oh, :ow] > 0.5
            st = RLE.statement(m)
            assert rows[b][j]['size'] == [oh, ow] and rows[b][j]['counts'] == st['chars'].decode('ascii'), (b, j)
            assert rows[b][j]['area'] == st['area'] == int(area[b, j]) and rows[b][j]['bbox'] == st['bbox'], (b, j)
            some = some or (0 < st['area'] < oh * ow)
        assert not _words(bits)[b, int(counts[b]):].any()        # padding detections
    assert some
    got = infer.mask_rows(bits, out[3], 500, status=status)
    assert got[0].shape == (counts[0], 320, 500) and np.array_equal(got[1][:, :150, :240], p['want'][TOP_N:TOP_N + counts[1], :150, :240] > 0.5)


def test_existing_entries_unchanged_and_predict_passes_the_argument(cuda, whole_pass):
    from scda_amd import infer
    p = whole_pass
    plain = infer.Predictor(p['det'], p['cfg'], masks=True, rle=True)(p['x'], p['info'])
    assert type(plain) is infer.PredictorResult and isinstance(plain, tuple) and len(plain) == 6
    assert plain.rle is plain[5] and plain.mask_bits is plain[4] and plain.mask_bits_orig is None and plain.orig_status is None
    for i in range(5):
        assert torch.equal(plain[i], p['out'][i]), i
    assert np.array_equal(plain[5]['size'].cpu().numpy(), [[256, 400], [240, 384]])      # without original_size: the input resolution
    no_rle = infer.Predictor(p['det'], p['cfg'], masks=True, original_size=(320, 512))(p['x'], p['info'])
    assert len(no_rle) == 8 and no_rle.rle is None and torch.equal(no_rle.mask_bits_orig, p['names']['mask_bits_orig'])
    for i in range(5):
        assert torch.equal(no_rle[i], p['out'][i]), i
    with pytest.raises(ValueError):
        infer.segm_rows(no_rle)
    again = infer.predict(p['det'], p['x'], p['info'], p['cfg'], masks=True, rle=True, original_size=(320, 512), rle_capacity=RLE_CAP)
    assert len(again) == 9 and torch.equal(again.mask_bits_orig, p['names']['mask_bits_orig'])
    assert torch.equal(again.det_orig, p['names']['det_orig'])
    with pytest.raises(ValueError):
        infer.Predictor(p['det'], p['cfg'], original_size=(320, 512))                     # needs masks=True
    with pytest.raises(ValueError):
        infer.Predictor(p['det'], p['cfg'], masks=True, original_size=(320, 512))(p['x'], p['info'][:, :3])


def test_flagged_image_raises_on_the_host(cuda, whole_pass):
    from scda_amd import infer
    p = whole_pass
    info = p['info'].clone()
    info[1, 3:5] = torch.tensor([400.0, 240.0])                  # above the capacity of 320 rows
    res = infer.Predictor(p['det'], p['cfg'], masks=True, rle=True, original_size=(320, 512), rle_capacity=RLE_CAP)(p['x'], info)
    assert res.orig_status.cpu().tolist() == [0, O.FLAG_CAPACITY]
    assert torch.equal(res.mask_bits_orig[0], p['names']['mask_bits_orig'][0]) and not res.mask_bits_orig[1].any()
    with pytest.raises(ValueError, match="status"):
        infer.segm_rows(res)
    with pytest.raises(ValueError, match="status"):
        infer.mask_rows(res.mask_bits_orig, res[3], status=res.orig_status)


def test_coco_stats_refuses_a_flagged_image(cuda, whole_pass):
    from scda_amd import evaluate, infer
    from scda_amd.coco_eval import CocoEvaluator
    p = whole_pass
    info = p['info'].clone()
    info[1, 3:5] = torch.tensor([400.0, 240.0])                  # above the capacity of 320 rows
    pred = infer.Predictor(p['det'], p['cfg'], masks=True, rle=True, original_size=(320, 512), rle_capacity=RLE_CAP)
    item = {'image': p['x'], 'image_info': info, 'image_ids': torch.tensor([12, 5], dtype=torch.int32), 'annotations': [[], []]}
    ev = CocoEvaluator(int(p['cfg']['shared']['num_classes']) - 1, 'bbox', max_images=2, max_dets_per_image=TOP_N, max_gts_per_image=4, device=cuda)
    with pytest.raises(ValueError, match=r"\(5, 1\)"):
        evaluate.coco_stats([item], pred, ev)


def test_replay_equals_eager(cuda, whole_pass):
    from scda_amd import infer
    from test_mask_infer_gpu import _images
    p = whole_pass
    info = p['info'].to(cuda)
    pred = infer.Predictor(p['det'], p['cfg'], masks=True, rle=True, original_size=(320, 512), rle_capacity=RLE_CAP)
    pred(_images(84, 2, cuda), info)
    pred.capture(_images(84, 2, cuda), info)
    pred.images.copy_(p['x'])
    got = pred.replay()
    torch.cuda.synchronize()
    assert len(got) == 9
    for i, (a, b) in enumerate(zip(got, p['out'])):
        if i == 5:
            n = b['n_bytes'].cpu().numpy()
            for k in ('n_runs', 'n_bytes', 'area', 'bbox', 'size'):
                assert torch.equal(a[k], b[k]), k
            ca, cb = a['chars'].cpu().numpy(), b['chars'].cpu().numpy()
            for bi in range(2):
                for j in range(TOP_N):
                    assert np.array_equal(ca[bi, j, :n[bi, j]], cb[bi, j, :n[bi, j]])
        else:
            assert torch.equal(a, b), i


def test_coco_stats_at_original_coordinates(cuda):
    """2 images, both down-scaled, ground truth at ORIGINAL coordinates cut from the pass's own original-size detections: coco_stats
    with original_size equals the route where this test resizes (the numpy statement), thresholds and matches on the host, and differs
    from the input-resolution route on the same data"""
    from scda_amd import evaluate, infer
    from scda_amd.coco_eval import CocoEvaluator
    from test_mask_infer_gpu import H_IMG, W_IMG, _images
    det, cfg = _detector(cuda)
    x = _images(71, 2, cuda)
    info = torch.tensor([[H_IMG, W_IMG, 1.6, 160, 250], [240, 384, 2.0, 120, 192]], dtype=torch.float32)
    sizes = [(160, 250), (120, 192)]
    pred = infer.Predictor(det, cfg, masks=True, rle=True, original_size=(160, 256))
    res = pred(x, info)
    counts = res[3].cpu().numpy()
    dets = res[2].cpu().numpy()
    K, G = int(cfg['shared']['num_classes']) - 1, 6
    O_all, _, status = O.statement(pred.mask_rois.cpu().numpy(), pred.mask_planes.cpu().numpy(), H_IMG, W_IMG, info.numpy(), TOP_N,
                                   160, 256, cls=pred.mask_cls.cpu().numpy())
    assert not status.any() and counts.min() >= 3
    host = []
    anns = []
    for b in range(2):
        oh, ow = sizes[b]
        n = int(counts[b])
        masks = O_all[b * TOP_N:b * TOP_N + n, :oh, :ow] > 0.5
        corners = dets[b, :n, 1:5] / info.numpy()[b, 2]
        xywh = cnp.xywh_from_corners(corners)
        gt_masks, a = [], []
        for g, j in enumerate(range(0, n, 3)):
            if g >= G:
                break
            m = masks[j].copy()                                  # the detection's own original-size mask without its first row
            set_rows = np.flatnonzero(m.any(1))
            if len(set_rows):
                m[set_rows[0]] = False
            gt_masks.append(m)
            a.append({'segmentation': {'size': [oh, ow], 'counts': [int(v) for v in RLE.encode(m)]},
                      'bbox': [float(xywh[j, 0] + 1), float(xywh[j, 1]), float(xywh[j, 2]), float(xywh[j, 3])],
                      'area': float(m.sum()), 'iscrowd': int(g == 1), 'category_id': int(dets[b, j, 6])})
        anns.append(a)
        host.append({'masks': masks, 'xywh': xywh, 'gt_masks': np.stack(gt_masks), 'n': n})
    item = {'image': x, 'image_info': info, 'image_ids': torch.tensor([12, 5], dtype=torch.int32), 'annotations': anns}
    plain = infer.Predictor(det, cfg, masks=True, rle=True)
    for iou_type in ('segm', 'bbox'):
        new = lambda: CocoEvaluator(K, iou_type, max_images=2, max_dets_per_image=TOP_N, max_gts_per_image=G, device=cuda)   # noqa: E731
        stats = evaluate.coco_stats([item], pred, new())        # 'sizes' come from image_info[:, 3:5]
        images = []
        for b in range(2):
            hb, a = host[b], anns[b]
            crowd = np.array([g['iscrowd'] for g in a], dtype=np.uint8)
            gt_xywh = np.array([g['bbox'] for g in a], dtype=np.float64)
            if iou_type == 'segm':
                iou, dt_area = RLE.iou(hb['masks'], hb['gt_masks'], crowd)[0], hb['masks'].reshape(hb['n'], -1).sum(1).astype(np.float64)
            else:
                iou, dt_area = cnp.bb_iou(hb['xywh'], gt_xywh, crowd), hb['xywh'][:, 2] * hb['xywh'][:, 3]
            images.append({'image_id': [12, 5][b], 'dt_xywh': hb['xywh'], 'dt_score': dets[b, :hb['n'], 5],
                           'dt_cat': dets[b, :hb['n'], 6].astype(np.int32), 'dt_area': dt_area, 'gt_xywh': gt_xywh,
                           'gt_area': np.array([g['area'] for g in a]), 'gt_iscrowd': crowd,
                           'gt_cat': np.array([g['category_id'] for g in a], dtype=np.int32), 'iou': iou})
        want = cnp.evaluate(images, K)
        n = cnp.stat_counts(want['precision'], want['recall'], want['specs'])
        print(iou_type, "stats", stats, "host", want['stats'])
        assert np.all(np.abs(stats - want['stats']) <= 2.0 * n * 2.0 ** -53) and stats[0] > 0, (iou_type, stats, want['stats'])
        # the parent's route on the same data: detections at the network input's coordinates against ground truth at the original's
        old = evaluate.coco_stats([dict(item, sizes=sizes)], plain, new())
        print(iou_type, "input-resolution route", old)
        assert not np.array_equal(old, stats), iou_type
