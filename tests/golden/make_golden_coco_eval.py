"""Generates tests/golden/coco_eval_ref.npz with the REFERENCE's evaluator: datasets/pycocotools/coco.py and cocoeval.py are imported
UNMODIFIED; the Cython module they expect (pycocotools._mask) is replaced in sys.modules by a stand-in whose iou / area / toBbox call the
reference's own datasets/pycocotools/common/maskApi.c (bbIou, rleIou, rleArea, rleToBbox), compiled with the system C compiler into a
temporary directory and reached over ctypes.  Run in the build container:
    python tests/golden/make_golden_coco_eval.py [path of the reference checkout]

Two shims for the toolchain's numpy: np.float = float, and np.linspace's `num` made an int (Params passes np.round(...) + 1, a float).
Neither the C file nor the library nor any reference program text is kept.  The file holds inputs and recorded outputs only, per set
`s` (flat over the images in the order they are GIVEN, cut by s_dt_counts / s_gt_counts):
  inputs    s_image_ids, s_K, s_area_rng [4, 2], s_dt_corners f32 [n, 4] (x1, y1, x2, y2; the reference sees x, y, (double) x2 - x1, ...),
            s_dt_scores f32, s_dt_cats, s_dt_areas f64, s_gt_boxes f64 [g, 4] xywh, s_gt_areas, s_gt_iscrowd, s_gt_cats; for 'segm' also
            s_dt_bits / s_gt_bits u32 [*, H, Wd] (packed as scda_mask_paste_hip packs) and s_size (h, w)
  recorded  s_iou (per image o[g * D + d] of every pair: bbIou / rleIou), s_rank (position under the evaluator's stable score sort within
            (image, category), -1 past maxDets[-1]), s_match i32 [n, A, T] (evalImgs' dtMatches as GT rows of the image, -1 = none), s_ignore u8
            [n, A, T] (dtIgnore), s_gt_ignore u8 [g, A] (gtIgnore), s_npig [K, A], s_precision, s_recall, s_scores (COCOeval.eval), s_stats
The sets (see main for the asserted coverage):
  rules        hand-made images, K = 4, image ids given in descending order
  random_bbox  40 images of 512 x 1024, K = 5, detections jittered from the GTs at three noise scales, 15 % crowds
  random_segm  12 images, planes 70 x 96 (Wd = 3), ellipses and blobs, K = 3, area ranges scaled to 8^2 / 24^2
  waves, capacity, limits, limits3, sortkeys, prrounds: the structural edge sets built by tests/eval_edge_cases.py, with their own
               s_iou_thrs, s_rec_thrs, s_max_dets and without s_iou
An array of the older sets must come out byte-identical; main asserts it before it writes."""
import ctypes
import importlib
import io
import contextlib
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import coco_eval_np as cnp  # noqa: E402  (parameters and the corner -> xywh rule only)
import eval_edge_cases as edges  # noqa: E402  (the seeded builders of the edge sets)


class RLE(ctypes.Structure):
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def load_maskapi(ref_root, tmp):
    common = os.path.join(ref_root, "datasets", "pycocotools", "common")
    so = os.path.join(tmp, "libmaskapi.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c99", "-I" + common, os.path.join(common, "maskApi.c"), "-o", so, "-lm"])
    return ctypes.CDLL(so)


def make_standin(lib):
    """pycocotools._mask over maskApi.c.  A mask object is {'size': [h, w], 'counts': bytes, 'mask': bool [h, w]}"""
    def rle_of(obj):
        m = np.asfortranarray(obj['mask'].astype(np.uint8))
        r = RLE()
        lib.rleEncode(ctypes.byref(r), m.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(m.shape[0]), ctypes.c_ulong(m.shape[1]), ctypes.c_ulong(1))
        return r

    def iou(dt, gt, pyiscrowd):
        m, n = len(dt), len(gt)
        if m == 0 or n == 0:
            return []
        crowd = np.ascontiguousarray(pyiscrowd, dtype=np.uint8)
        o = np.zeros(n * m, dtype=np.float64)
        if isinstance(dt[0], dict):
            D = (RLE * m)(*[rle_of(x) for x in dt])
            G = (RLE * n)(*[rle_of(x) for x in gt])
            lib.rleIou(D, G, ctypes.c_ulong(m), ctypes.c_ulong(n), crowd.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p))
        else:
            d = np.ascontiguousarray(dt, dtype=np.float64).reshape(m, 4)
            g = np.ascontiguousarray(gt, dtype=np.float64).reshape(n, 4)
            lib.bbIou(d.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(m), ctypes.c_ulong(n),
                      crowd.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p))
        return o.reshape(n, m).T.copy()

    def area(objs):
        out = []
        for x in objs:
            a = ctypes.c_uint(0)
            r = rle_of(x)
            lib.rleArea(ctypes.byref(r), ctypes.c_ulong(1), ctypes.byref(a))
            out.append(a.value)
        return np.asarray(out, dtype=np.uint32)

    def to_bbox(objs):
        out = np.zeros((len(objs), 4), dtype=np.float64)
        for i, x in enumerate(objs):
            bb = (ctypes.c_double * 4)()
            r = rle_of(x)
            lib.rleToBbox(ctypes.byref(r), bb, ctypes.c_ulong(1))
            out[i] = list(bb)
        return out

    def unsupported(*a, **k):
        raise NotImplementedError("not needed by COCOeval on ready-made masks")

    mod = types.ModuleType("pycocotools._mask")
    mod.iou, mod.area, mod.toBbox = iou, area, to_bbox
    mod.merge = mod.frPyObjects = mod.encode = mod.decode = unsupported
    return mod


def import_reference(ref_root, standin):
    np.float = float                                                          # (numpy >= 1.24 dropped the alias cocoeval.py uses)
    linspace = np.linspace
    np.linspace = lambda start, stop, num=50, *a, **k: linspace(start, stop, int(num), *a, **k)
    pkg = types.ModuleType("pycocotools")
    pkg.__path__ = [os.path.join(ref_root, "datasets", "pycocotools")]
    sys.modules["pycocotools"] = pkg
    sys.modules["pycocotools._mask"] = standin
    return importlib.import_module("pycocotools.coco"), importlib.import_module("pycocotools.cocoeval")


def pack(mask, H, Wd):
    full = np.zeros((H, Wd * 32), dtype=np.uint8)
    full[:mask.shape[0], :mask.shape[1]] = mask
    return np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(H, Wd)


def run_reference(coco_mod, eval_mod, standin, images, K, area_rng, iou_type, size, params=None):
    """images: dicts with image_id, dt_corners, dt_score, dt_cat, gt_xywh, gt_area, gt_iscrowd, gt_cat (+ dt_mask, gt_mask for segm);
    params: iou_thrs, rec_thrs and max_dets other than Params' defaults (the edge sets)"""
    h, w = size
    gt_anns, dt_anns = [], []
    for im in images:
        xywh = cnp.xywh_from_corners(im['dt_corners'])
        im['dt_first'], im['gt_first'] = len(dt_anns), len(gt_anns)
        for g in range(len(im['gt_cat'])):
            ann = {'id': len(gt_anns) + 1, 'image_id': im['image_id'], 'category_id': int(im['gt_cat'][g]),
                   'bbox': [float(v) for v in im['gt_xywh'][g]], 'area': float(im['gt_area'][g]), 'iscrowd': int(im['gt_iscrowd'][g])}
            if iou_type == 'segm':
                ann['segmentation'] = {'size': [h, w], 'counts': b'', 'mask': im['gt_mask'][g]}
            gt_anns.append(ann)
        for d in range(len(im['dt_score'])):
            ann = {'image_id': im['image_id'], 'category_id': int(im['dt_cat'][d]), 'score': float(im['dt_score'][d])}
            if iou_type == 'segm':
                ann['segmentation'] = {'size': [h, w], 'counts': b'', 'mask': im['dt_mask'][d]}
            else:
                ann['bbox'] = [float(v) for v in xywh[d]]
            dt_anns.append(ann)
    gt = coco_mod.COCO()
    gt.dataset = {'images': [{'id': im['image_id'], 'height': h, 'width': w} for im in images],
                  'categories': [{'id': k} for k in range(1, K + 1)], 'annotations': gt_anns}
    with contextlib.redirect_stdout(io.StringIO()):
        gt.createIndex()
        dt = gt.loadRes(dt_anns)
        E = eval_mod.COCOeval(gt, dt, iou_type)
        E.params.areaRng = [list(map(float, r)) for r in area_rng]
        E.params.areaRngLbl = ['all', 'small', 'medium', 'large'] + ['range%d' % a for a in range(4, len(area_rng))]
        if params is not None:
            E.params.iouThrs, E.params.recThrs = np.asarray(params['iou_thrs']), np.asarray(params['rec_thrs'])
            E.params.maxDets = list(params['max_dets'])
        E.evaluate()
        E.accumulate()
        E.summarize()
    # ---- the recorded arrays
    T, A = len(E.params.iouThrs), len(area_rng)
    nd, ng = len(dt_anns), len(gt_anns)
    rank = np.full(nd, -1, dtype=np.int32)
    match = np.full((nd, A, T), -1, dtype=np.int32)
    ignore = np.zeros((nd, A, T), dtype=np.uint8)
    gt_ignore = np.zeros((ng, A), dtype=np.uint8)
    npig = np.zeros((K, A), dtype=np.int32)
    first_gt = {im['image_id']: im['gt_first'] for im in images}
    ids = sorted(im['image_id'] for im in images)
    I = len(ids)
    for k in range(K):
        for a in range(A):
            for i in range(I):
                e = E.evalImgs[(k * A + a) * I + i]
                if e is None:
                    continue
                assert e['image_id'] == ids[i] and e['category_id'] == k + 1
                di = np.asarray(e['dtIds'], dtype=np.int64) - 1
                gi = np.asarray(e['gtIds'], dtype=np.int64) - 1
                rank[di] = np.arange(len(di))
                m = e['dtMatches'].astype(np.int64)                           # [T, D]: GT ids, 0 = none
                match[di, a, :] = np.where(m > 0, m - 1 - first_gt[e['image_id']], -1).T
                ignore[di, a, :] = np.asarray(e['dtIgnore']).astype(np.uint8).T
                gt_ignore[gi, a] = np.asarray(e['gtIgnore']).astype(np.uint8)
                npig[k, a] += int((np.asarray(e['gtIgnore']) == 0).sum())
    # every pair's IoU of an image, from the same C
    iou = []
    for im in images:
        D, G = len(im['dt_score']), len(im['gt_cat'])
        if D == 0 or G == 0:
            continue
        if iou_type == 'segm':
            d = [{'mask': x} for x in im['dt_mask']]; g = [{'mask': x} for x in im['gt_mask']]
        else:
            d = cnp.xywh_from_corners(im['dt_corners']); g = im['gt_xywh']
        iou.append(standin.iou(d, g, im['gt_iscrowd']).T.reshape(-1))          # [G, D]
    out = {'rank': rank, 'match': match, 'ignore': ignore, 'gt_ignore': gt_ignore, 'npig': npig,
           'iou': np.concatenate(iou) if iou else np.zeros(0), 'precision': E.eval['precision'], 'recall': E.eval['recall'],
           'scores': E.eval['scores'], 'stats': np.asarray(E.stats, dtype=np.float64)}
    if iou_type == 'segm':
        out['dt_areas'] = np.concatenate([standin.area([{'mask': x} for x in im['dt_mask']]).astype(np.float64) if len(im['dt_mask'])
                                          else np.zeros(0) for im in images])
    return out


def image(image_id, dets, gts):
    """dets: (x1, y1, x2, y2, score, cat); gts: (x, y, w, h, iscrowd, cat[, area])"""
    d = np.asarray(dets, dtype=np.float64).reshape(-1, 6)
    g = [tuple(r) + ((r[2] * r[3],) if len(r) == 6 else ()) for r in gts]
    g = np.asarray(g, dtype=np.float64).reshape(-1, 7)
    return {'image_id': image_id, 'dt_corners': d[:, :4].astype(np.float32), 'dt_score': d[:, 4].astype(np.float32),
            'dt_cat': d[:, 5].astype(np.int32), 'gt_xywh': g[:, :4].copy(), 'gt_area': g[:, 6].copy(),
            'gt_iscrowd': g[:, 4].astype(np.uint8), 'gt_cat': g[:, 5].astype(np.int32)}


def rules_set(rng):
    ims = []
    # 90: a crowd GT that two detections match; a regular GT beside it
    ims.append(image(90, [(12, 12, 30, 30, .9, 1), (20, 20, 35, 35, .8, 1), (100, 100, 140, 140, .7, 1)],
                     [(10, 10, 50, 50, 1, 1), (100, 100, 40, 40, 0, 1)]))
    # 80: the break: a regular match (IoU 10/12) is held when the crowd GT behind it offers IoU 1
    ims.append(image(80, [(0, 0, 10, 10, .95, 1)], [(0, 0, 10, 10, 1, 1), (0, 0, 10, 12, 0, 1)]))
    # 70: IoU exactly 0.5
    ims.append(image(70, [(0, 0, 1, 1, .6, 1)], [(0, 0, 2, 1, 0, 1)]))
    # 60: two GTs with the same IoU 80 / 120: the later one is matched.  A score tie with image 50
    ims.append(image(60, [(10, 10, 20, 20, 1.0, 1)], [(8, 10, 10, 10, 0, 1), (12, 10, 10, 10, 0, 1)]))
    # 50: areas exactly 32^2 and 96^2 (inside 'small' and 'medium', and 'medium' and 'large'); two scores tied at 1.0
    ims.append(image(50, [(0, 0, 32, 32, 1.0, 1), (100, 100, 196, 196, 1.0, 1)], [(0, 0, 32, 32, 0, 1), (100, 100, 96, 96, 0, 1)]))
    # 40: an unmatched detection of area 25 (outside 'medium' and 'large'), a GT nobody finds
    ims.append(image(40, [(200, 200, 205, 205, .5, 1)], [(20, 20, 50, 50, 0, 1)]))
    # 30: category 2 has GTs only, category 3 detections only; category 4 never occurs
    ims.append(image(30, [(5, 5, 60, 60, .4, 3), (50, 50, 90, 90, .3, 3)], [(5, 5, 55, 55, 0, 2), (300, 100, 120, 130, 0, 2)]))
    # 20: nothing
    ims.append(image(20, [], []))
    # 10: 120 detections of one category (ranks past the cut of 100), tied scores among them
    gts = [(40.0 * j, 30.0, 30.0 + 6 * j, 30.0 + 7 * j, 1 if j == 5 else 0, 1) for j in range(10)]
    dets = []
    for j in range(120):
        g = gts[j % 10]
        dx, dy = rng.randint(-6, 7, 2)
        dets.append((g[0] + dx, g[1] + dy, g[0] + dx + g[2] + rng.randint(-4, 5), g[1] + dy + g[3] + rng.randint(-4, 5),
                     np.round(rng.uniform(0.05, 1.0), 2), 1))
    ims.append(image(10, dets, gts))
    return ims


def random_bbox_set(rng, n_images=40, H=512, W=1024, K=5):
    ims = []
    for i in range(n_images):
        G = rng.randint(3, 13)
        w = np.exp(rng.uniform(np.log(8), np.log(400), G)); h = np.exp(rng.uniform(np.log(8), np.log(300), G))
        x = rng.uniform(0, W - w); y = rng.uniform(0, H - h)
        gts = [(np.round(x[g], 1), np.round(y[g], 1), np.round(w[g], 1), np.round(h[g], 1), int(rng.rand() < 0.15), rng.randint(1, K + 1))
               for g in range(G)]
        gts = [g + (g[2] * g[3] * rng.choice([0.6, 1.0]),) for g in gts]
        dets = []
        for _ in range(rng.randint(20, 101)):
            g = gts[rng.randint(G)]
            s = rng.choice([0.03, 0.12, 0.4])
            x1 = g[0] + rng.normal(0, s) * g[2]; y1 = g[1] + rng.normal(0, s) * g[3]
            ww = g[2] * np.exp(rng.normal(0, s)); hh = g[3] * np.exp(rng.normal(0, s))
            cat = g[5] if rng.rand() < 0.85 else rng.randint(1, K + 1)
            dets.append((x1, y1, x1 + ww, y1 + hh, np.round(rng.uniform(0.05, 1.0), 2), cat))
        ims.append(image(1000 + int(rng.randint(0, 100000)) * 40 + i, dets, gts))
    return ims


def random_segm_set(rng, n_images=12, h=70, w=96, K=3):
    yy, xx = np.mgrid[:h, :w]

    def shape(cx, cy, rx, ry, blob):
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        if blob:
            coarse = rng.rand(6, 8)
            field = np.kron(coarse, np.ones((12, 12)))[:h, :w]
            m = m & (field > 0.25)
        return m

    ims = []
    for i in range(n_images):
        G = rng.randint(2, 7)
        gm, gts, dets, dm = [], [], [], []
        for g in range(G):
            cx, cy = rng.uniform(5, w - 5), rng.uniform(5, h - 5)
            rx, ry = np.exp(rng.uniform(np.log(1.5), np.log(30))), np.exp(rng.uniform(np.log(1.5), np.log(25)))
            m = shape(cx, cy, rx, ry, rng.rand() < 0.4)
            if not m.any():
                m[int(cy), int(cx)] = True
            cat = rng.randint(1, K + 1)
            gm.append(m)
            gts.append((0, 0, 0, 0, int(rng.rand() < 0.15), cat, float(m.sum()) * rng.choice([0.6, 1.0])))
            for _ in range(rng.randint(1, 5)):
                s = rng.choice([0.03, 0.12, 0.4])
                mm = shape(cx + rng.normal(0, s) * rx, cy + rng.normal(0, s) * ry, rx * np.exp(rng.normal(0, s)),
                           ry * np.exp(rng.normal(0, s)), rng.rand() < 0.3)
                dm.append(mm)
                dets.append((0, 0, 0, 0, np.round(rng.uniform(0.05, 1.0), 1), cat if rng.rand() < 0.85 else rng.randint(1, K + 1)))
        im = image(7 * (n_images - i) + 3, dets, gts)
        im['gt_mask'], im['dt_mask'] = gm, dm
        ims.append(im)
    return ims


def store(out, name, images, K, area_rng, rec, size=None):
    cat = lambda key, dt, width=None: (np.concatenate([im[key] for im in images]) if images else np.zeros(0)).astype(dt)   # noqa: E731
    out[name + '_image_ids'] = np.asarray([im['image_id'] for im in images], dtype=np.int32)
    out[name + '_K'] = np.asarray(K, dtype=np.int32)
    out[name + '_area_rng'] = np.asarray(area_rng, dtype=np.float64)
    out[name + '_dt_counts'] = np.asarray([len(im['dt_score']) for im in images], dtype=np.int32)
    out[name + '_gt_counts'] = np.asarray([len(im['gt_cat']) for im in images], dtype=np.int32)
    out[name + '_dt_corners'] = cat('dt_corners', np.float32).reshape(-1, 4)
    out[name + '_dt_scores'] = cat('dt_score', np.float32)
    out[name + '_dt_cats'] = cat('dt_cat', np.int32)
    out[name + '_gt_boxes'] = cat('gt_xywh', np.float64).reshape(-1, 4)
    out[name + '_gt_areas'] = cat('gt_area', np.float64)
    out[name + '_gt_iscrowd'] = cat('gt_iscrowd', np.uint8)
    out[name + '_gt_cats'] = cat('gt_cat', np.int32)
    if size is None:
        xywh = cnp.xywh_from_corners(out[name + '_dt_corners'])
        out[name + '_dt_areas'] = xywh[:, 2] * xywh[:, 3]
    else:
        H, Wd = size[0], (size[1] + 31) // 32
        out[name + '_size'] = np.asarray(size, dtype=np.int32)
        out[name + '_dt_bits'] = np.stack([pack(m, H, Wd) for im in images for m in im['dt_mask']])
        out[name + '_gt_bits'] = np.stack([pack(m, H, Wd) for im in images for m in im['gt_mask']])
        out[name + '_dt_areas'] = rec.pop('dt_areas')
    for k, v in rec.items():
        out[name + '_' + k] = v


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SCDA_REFERENCE", "/root/reference")
    rng = np.random.RandomState(2017)
    params = cnp.default_params()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        standin = make_standin(load_maskapi(ref_root, tmp))
        coco_mod, eval_mod = import_reference(ref_root, standin)
        P = eval_mod.Params('bbox')
        assert np.array_equal(P.iouThrs, params['iou_thrs']) and np.array_equal(P.recThrs, params['rec_thrs'])
        assert P.maxDets == params['max_dets'] and np.array_equal(np.asarray(P.areaRng, dtype=np.float64), params['area_rng'])

        # ---- rules
        ims = rules_set(rng)
        assert [im['image_id'] for im in ims] == sorted((im['image_id'] for im in ims), reverse=True)
        r = run_reference(coco_mod, eval_mod, standin, ims, 4, params['area_rng'], 'bbox', (512, 1024))
        store(out, 'rules', ims, 4, params['area_rng'], dict(r))
        first = {im['image_id']: im['dt_first'] for im in ims}
        m90 = r['match'][first[90]:first[90] + 2, 0, 0]
        assert m90[0] == 0 and m90[1] == 0, "the crowd GT must take two detections"
        assert r['match'][first[80], 0, 0] == 1 and r['iou'].max() == 1.0, "the break case must keep the regular match"
        assert r['match'][first[80], 0, 9] == 0 and r['ignore'][first[80], 0, 9] == 1
        assert (r['iou'] == 0.5).any() and r['match'][first[70], 0, 0] == 0, "IoU exactly 0.5 must match at threshold 0.5"
        assert r['match'][first[60], 0, 0] == 1, "of two GTs with equal IoU the later one wins"
        assert r['gt_ignore'][ims[4]['gt_first']].tolist() == [0, 0, 0, 1] and r['gt_ignore'][ims[4]['gt_first'] + 1].tolist() == [0, 1, 0, 0]
        assert r['match'][first[40], 0, 0] == -1 and r['ignore'][first[40], :, 0].tolist() == [0, 0, 1, 1]
        assert (out['rules_dt_scores'] == 1.0).sum() >= 3
        assert (r['precision'][:, :, 1, 0] == 0).all() and (r['recall'][:, 1, 0] == 0).all() and r['npig'][1, 0] == 2, "GTs only: zeros"
        assert (r['precision'][:, :, 1, 1] == -1).all() and (r['precision'][:, :, 2:] == -1).all(), "npig == 0 / never seen: -1"
        assert r['rank'][first[10]:first[10] + 120].max() == 99 and (r['rank'][first[10]:first[10] + 120] == -1).sum() == 20
        print("rules stats", np.round(r['stats'], 4))

        # ---- random_bbox
        ims = random_bbox_set(rng)
        r = run_reference(coco_mod, eval_mod, standin, ims, 5, params['area_rng'], 'bbox', (512, 1024))
        store(out, 'random_bbox', ims, 5, params['area_rng'], dict(r))
        assert (r['stats'] > -1).all(), r['stats']
        sc = np.concatenate([im['dt_score'] for im in ims])
        assert len(np.unique(sc)) < len(sc), "a score tie must be present"
        print("random_bbox stats", np.round(r['stats'], 4), "gts", sum(len(im['gt_cat']) for im in ims), "dets", len(sc))

        # ---- random_segm
        ims = random_segm_set(rng)
        rng_s = np.array([[0, 1e10], [0, 8 ** 2], [8 ** 2, 24 ** 2], [24 ** 2, 1e10]], dtype=np.float64)
        r = run_reference(coco_mod, eval_mod, standin, ims, 3, rng_s, 'segm', (70, 96))
        # the boxes of the masks (not used by the 'segm' evaluation; kept so that the rows are complete)
        for im in ims:
            bb = standin.toBbox([{'mask': m} for m in im['gt_mask']]) if im['gt_mask'] else np.zeros((0, 4))
            im['gt_xywh'] = bb
            db = standin.toBbox([{'mask': m} for m in im['dt_mask']]) if im['dt_mask'] else np.zeros((0, 4))
            im['dt_corners'] = np.stack([db[:, 0], db[:, 1], db[:, 0] + db[:, 2], db[:, 1] + db[:, 3]], 1).astype(np.float32)
        store(out, 'random_segm', ims, 3, rng_s, dict(r), size=(70, 96))
        assert (r['stats'] > -1).all(), r['stats']
        sc = np.concatenate([im['dt_score'] for im in ims])
        assert len(np.unique(sc)) < len(sc)
        print("random_segm stats", np.round(r['stats'], 4), "gts", sum(len(im['gt_cat']) for im in ims), "dets", len(sc))
        # ---- the edge sets of tests/eval_edge_cases.py (test_eval_edges_rules.py asserts the boundary each one crosses); their IoU
        # matrices are not stored: cnp.bb_iou recomputes them
        for name in edges.COCO_SETS:
            case = edges.coco_case(name)
            p = case['params']
            assert name + '_K' not in out and list(p['max_dets']) == sorted(p['max_dets'])
            r = run_reference(coco_mod, eval_mod, standin, case['images'], case['K'], p['area_rng'], 'bbox', (1024, 1024), p)
            r.pop('iou')
            store(out, name, case['images'], case['K'], p['area_rng'], dict(r))
            out[name + '_iou_thrs'], out[name + '_rec_thrs'] = np.asarray(p['iou_thrs'], np.float64), np.asarray(p['rec_thrs'], np.float64)
            out[name + '_max_dets'] = np.asarray(p['max_dets'], dtype=np.int32)
            print(name, "stats", np.round(r['stats'], 4), "gts", len(out[name + '_gt_cats']), "dets", len(out[name + '_dt_cats']))
    path = os.path.join(HERE, "coco_eval_ref.npz")
    if os.path.exists(path):                                                  # regeneration must not move an array of the older sets
        with np.load(path) as old:
            for k in (k for k in old.files if not any(k.startswith(s + '_') for s in edges.COCO_SETS)):
                assert out[k].dtype == old[k].dtype and out[k].shape == old[k].shape and out[k].tobytes() == old[k].tobytes(), k
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
