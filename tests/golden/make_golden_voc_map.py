"""Generates tests/golden/voc_map_ref.npz with the REFERENCE's metric: utils/cal_mAP.py is imported UNMODIFIED (parse_gts, parse_res,
cal_mAP) and bbox_helper.compute_recall is reached through tests/golden/ref_harness.py.  Run in the build container:
    python tests/golden/make_golden_voc_map.py [path of the reference checkout]

The text rows the reference parses are produced here from the detections by rule R1 of include/scda_ops.h restated with numpy float32
clip, `/` and str -- validate()'s own formatting (tools/faster_rcnn_train_val.py:838-857), except that the keep_num best rows are taken
with equal scores in the given order (validate()'s argsort()[::-1] orders equal scores as numpy happens to).  One shim: a class without
any row makes the reference's cal_mAP raise ValueError (np.max of an empty array; asserted here), so the module's `np` is replaced by a
proxy whose max() of an empty array is 0 -- the class's ap stays the zero it was initialised with, which is what the device path states.

No reference program text is kept.  The file holds inputs and recorded outputs only, per set `s` (flat over the images in the order they
are added, cut by the per-image counts):
  inputs    s_C, s_names, s_info f32 [I, 3] = (h, w, scale), s_det f32 [n, 7] and s_det_counts, s_gt i32 [g, 5] = (x1, y1, x2, y2,
            label) and s_gt_counts (0 for an image the meta does not have), s_in_meta u8 [I], s_sum_gt (the meta's gts['num'], images
            that are never added included); for the recall s_props f32 [p, 6], s_prop_counts, s_rgts f32 [r, 5], s_rgt_counts
  recorded  s_res i32 [m, 6] = (class, image, x1, y1, x2, y2) and s_res_score f64 [m]: parse_res' lists, class by class in file order;
            s_ap, s_max_recall, s_mAP (cal_mAP); s_is_det u8 [g] (gts[...]['is_det'] after cal_mAP, per ground-truth row);
            s_recalled, s_rpn_gts (compute_recall summed); s_tp u8 [n], s_match i32 [n] (tests/voc_map_np.py, after its ap / max_recall
            were asserted bit-equal to the reference's and its true positives per class equal to the is_det sums)
The sets (see main for the asserted coverage): rules (hand-made, C = 5), nan (a class with rows and no ground truth), random (40 images
of 512 x 1024 at scale 0.5, C = 9); cap, keep100, match, recall: the structural edge sets built by tests/eval_edge_cases.py, each with
s_keep_num (and, for the recall, s_recalled_each i32 [I, 2]).  An array of the older sets must come out byte-identical; main
asserts it before it writes."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import voc_map_np as vnp  # noqa: E402
import eval_edge_cases as edges  # noqa: E402  (the seeded builders of the edge sets)


class _NumpyEmptyMax:
    """numpy, with max() of an empty array = 0 (see the module docstring)"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def max(a, *args, **kw):
        return np.float64(0.0) if np.size(a) == 0 else np.max(a, *args, **kw)


def load_cal_map(ref_root):
    spec = importlib.util.spec_from_file_location("_ref_cal_mAP", os.path.join(ref_root, "utils", "cal_mAP.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def f32(*v):
    return np.asarray(v, dtype=np.float32)


def det_rows(rows):
    """[(x1, y1, x2, y2, score, class)] -> float32 [n, 7]"""
    out = np.zeros((len(rows), 7), dtype=np.float32)
    if rows:
        out[:, 1:] = np.asarray(rows, dtype=np.float32)
    return out


def text_rows(im, num_classes, keep_num=100):
    """R1 in numpy float32, formatted as validate() formats: the rows of one image"""
    det, info = im['det'], im['info']
    order = np.argsort(-det[:, 5].astype(np.float64), kind='stable')[:keep_num]
    top = det[order]
    out = []
    for c in range(1, num_classes):
        d = top[top[:, 6] == c][:, 1:6].copy()
        h, w = info[0], info[1]
        for col, hi in ((0, w - 1), (1, h - 1), (2, w - 1), (3, h - 1)):
            d[:, col] = np.clip(d[:, col], 0, hi)
        if len(d):
            d[:, :4] = d[:, :4] / info[-1]
        assert d.dtype == np.float32
        for bx in d:
            out.append('{0} {1} {2}\n'.format(im['name'], ' '.join(map(str, bx)), c))
    return out


def meta_lines(records):
    """[(name, gt int [g, 5])] -> the meta file's lines in the layout parse_gts reads"""
    out = []
    for k, (name, gt) in enumerate(records):
        out += ['# %d\n' % k, 'val/city/%s.png\n' % name, '3\n', '200\n', '400\n', '0\n', '0\n', '%d\n' % len(gt)]
        out += ['%d %d %d %d %d\n' % (g[4], g[0], g[1], g[2], g[3]) for g in gt]
    return out


def scale13_coordinate():
    """a float32 x whose float32 quotient by float32(1.3) truncates differently from the float64 quotient: the division must be the
    correctly rounded float32 one"""
    s = np.float32(1.3)
    for k in range(2, 190):
        x = np.float32(k) * s
        if int(x / s) != int(float(x) / float(s)):
            return x, int(x / s)
    raise AssertionError("no such coordinate")


def grid_gt(j, label=1):
    return [20 * (j % 16), 20 * (j // 16), 20 * (j % 16) + 9, 20 * (j // 16) + 9, label]


def rules_set():
    """-> (images to add, meta records, C)"""
    E = np.zeros((0, 5), dtype=np.int32)
    gt = lambda *rows: np.asarray(rows, dtype=np.int32).reshape(-1, 5)        # noqa: E731
    info1 = f32(200, 400, 1.0)
    images = []
    # IoU exactly 0.5; touching boxes; a one-pixel-wide detection; classes validate() never writes; the single row of class 3
    images.append({'name': 'a_half', 'info': info1,
                   'gt': gt([0, 0, 9, 19, 1], [50, 50, 60, 60, 1], [120, 40, 159, 79, 3]),
                   'det': det_rows([(0, 0, 9, 9, .9, 1), (60, 50, 70, 60, .8, 1), (52, 50, 52, 60, .7, 1), (120, 40, 159, 79, .77, 3),
                                    (300, 100, 320, 120, .99, 0), (300, 100, 320, 120, .98, 5), (300, 100, 320, 120, .97, 7)])})
    # a claimed ground truth is not given twice although another one is free; equal IoU: the first wins
    images.append({'name': 'b_claimed', 'info': info1,
                   'gt': gt([10, 10, 49, 49, 1], [10, 10, 49, 69, 1], [100, 10, 119, 29, 1], [100, 10, 119, 29, 1]),
                   'det': det_rows([(10, 10, 49, 49, .95, 1), (10, 10, 49, 51, .91, 1), (10, 10, 49, 69, .5, 1),
                                    (100, 10, 119, 29, .85, 1), (100, 10, 119, 29, .84, 1)])})
    # truncation: (0.9, 0.9, 9.9, 9.9) -> (0, 0, 9, 9), IoU 0.5 with (0, 0, 9, 19); rounding would give (1, 1, 10, 10) and 90 / 210
    images.append({'name': 'c_trunc', 'info': info1, 'gt': gt([0, 0, 9, 19, 1]), 'det': det_rows([(.9, .9, 9.9, 9.9, .66, 1), (10.9, 30.2, 40.9, 60.7, .2, 2)])})
    # clipping to w - 1 / h - 1 BEFORE the division, scale 0.5: x2 250 -> 199 -> 398; y1 -3 -> 0
    images.append({'name': 'd_clip', 'info': f32(100, 200, .5), 'gt': gt([300, 20, 398, 100, 1], [100, 0, 140, 198, 1]),
                   'det': det_rows([(150.2, 10.3, 250, 50.4, .88, 1), (50.2, -3, 70.4, 120, .87, 1)])})
    # scale 1.3
    x, k = scale13_coordinate()
    images.append({'name': 'e_scale13', 'info': f32(130, 260, 1.3), 'gt': gt([10, 20, k, 70, 1], [k - 5, 5, k + 30, 60, 2]),
                   'det': det_rows([(13.0, 26.0, x, 91.0, .81, 1), (39.0, 26.3, 117.1, 91.9, .3, 1)])})
    # equal scores inside an image (both rows best on the one ground truth: the earlier row takes it) and across images (f before g)
    images.append({'name': 'f_ties', 'info': info1, 'gt': gt([200, 100, 239, 139, 1]),
                   'det': det_rows([(200, 100, 239, 141, .6, 1), (200, 100, 239, 139, .6, 1), (5, 5, 30, 30, .6, 1)])})
    images.append({'name': 'g_ties', 'info': info1, 'gt': gt([200, 100, 239, 139, 1]),
                   'det': det_rows([(300, 5, 330, 30, .6, 1), (200, 100, 239, 139, .6, 1)])})
    # 130 rows, given unsorted; ten rows share the score at the 100 / 101 cut: 98 above them, the first two of the ten are kept
    rs = np.random.RandomState(7)
    rows = [(5 + 2 * i, 150, 25 + 2 * i, 190, .31 + .005 * (i + 1), 2 if i % 9 else 6) for i in range(98)]
    tied = [(5, 5, 30, 30, .3, 1), (40, 5, 60, 30, .3, 2), (100, 50, 139, 89, .3, 1), (100, 50, 139, 89, .3, 1)] + \
           [(5 + i, 100, 30 + i, 130, .3, 1) for i in range(6)]
    low = [(5 + i, 100, 30 + i, 130, .01 + .01 * i, 1) for i in range(22)]
    perm = rs.permutation(98)
    mixed = [rows[i] for i in perm[:50]] + tied[:3] + [rows[i] for i in perm[50:]] + low[:10] + tied[3:] + low[10:]
    images.append({'name': 'h_130', 'info': info1, 'gt': gt([100, 50, 139, 89, 1], [300, 20, 340, 60, 2]), 'det': det_rows(mixed)})
    # no ground truth; no detections; absent from the meta (only rows validate() never writes); never added (in the meta only)
    images.append({'name': 'i_no_gt', 'info': info1, 'gt': E, 'det': det_rows([(5, 5, 30, 30, .45, 1), (5, 5, 30, 30, .44, 2)])})
    images.append({'name': 'j_no_det', 'info': info1, 'gt': gt([5, 5, 30, 30, 1], [50, 5, 90, 30, 2], [50, 50, 90, 90, 4]), 'det': det_rows([])})
    images.append({'name': 'k_absent', 'info': info1, 'gt': E, 'in_meta': False, 'det': det_rows([(5, 5, 30, 30, .9, 0), (5, 5, 30, 30, .8, 5)])})
    # the wave boundary of the argmax: 63, 64 and 65 ground truths of class 1 (w65: a class-4 row first, so rows and class indices differ)
    g63 = [grid_gt(j) for j in range(63)]
    images.append({'name': 'w63', 'info': info1, 'gt': gt(*g63), 'det': det_rows([tuple(grid_gt(62)[:4]) + (.71, 1), tuple(grid_gt(0)[:4]) + (.72, 1)])})
    g64 = [grid_gt(j) for j in range(64)]
    images.append({'name': 'w64', 'info': info1, 'gt': gt(*g64), 'det': det_rows([tuple(grid_gt(63)[:4]) + (.73, 1), (300, 80, 309, 90, .74, 1)])})
    g65 = [[380, 180, 390, 190, 4]] + [grid_gt(j) for j in range(63)] + [[340, 100, 359, 119, 1], [350, 100, 369, 119, 1]]
    images.append({'name': 'w65', 'info': info1, 'gt': gt(*g65),
                   'det': det_rows([(340, 100, 359, 119, .78, 1), (350, 100, 369, 119, .76, 1), (345, 100, 364, 119, .79, 1)])})
    records = [(im['name'], im['gt']) for im in images if im.get('in_meta', True)]
    records.insert(3, ('never_added', gt([5, 5, 30, 30, 1], [5, 50, 30, 90, 1], [50, 50, 90, 90, 4])))
    return images, records, 5


def nan_set():
    gt = lambda *rows: np.asarray(rows, dtype=np.int32).reshape(-1, 5)        # noqa: E731
    info = f32(200, 400, 1.0)
    images = [{'name': 'n0', 'info': info, 'gt': gt([10, 10, 49, 49, 1]), 'det': det_rows([(10, 10, 49, 49, .9, 1), (100, 100, 140, 140, .8, 2)])},
              {'name': 'n1', 'info': info, 'gt': gt([10, 10, 49, 49, 1]), 'det': det_rows([(12, 10, 49, 49, .7, 1), (10, 10, 49, 49, .6, 2)])}]
    return images, [(im['name'], im['gt']) for im in images], 3


def random_set():
    rs = np.random.RandomState(20240607)
    C, H, W, scale = 9, 512, 1024, np.float32(.5)
    images = []
    for i in range(40):
        g = rs.randint(3, 31)
        w, h = rs.randint(24, 400, g), rs.randint(24, 300, g)
        x1, y1 = rs.randint(0, 2048 - w), rs.randint(0, 1024 - h)
        gt = np.stack([x1, y1, x1 + w, y1 + h, rs.randint(1, C, g)], 1).astype(np.int32)
        n = rs.randint(20, 101)
        src = rs.randint(0, g, n)
        noise = rs.choice([.02, .12, .4], n)[:, None] * np.stack([w[src], h[src], w[src], h[src]], 1)
        box = (gt[src, :4] + rs.uniform(-1, 1, (n, 4)) * noise) * .5 + rs.uniform(0, 1, (n, 4))
        box = np.stack([np.minimum(box[:, 0], box[:, 2]), np.minimum(box[:, 1], box[:, 3]), np.maximum(box[:, 0], box[:, 2]),
                        np.maximum(box[:, 1], box[:, 3])], 1)
        cls = np.where(rs.uniform(size=n) < .15, rs.randint(1, C, n), gt[src, 4])
        det = np.zeros((n, 7), dtype=np.float32)
        det[:, 1:5], det[:, 5], det[:, 6] = box, np.round(rs.uniform(.05, 1, n), 2), cls
        p = 0 if i == 5 else 64
        psrc = rs.randint(0, g, p)
        pb = gt[psrc, :4] * .5 + rs.uniform(-1, 1, (p, 4)) * rs.choice([2., 15., 60.], p)[:, None]
        props = np.zeros((p, 6), dtype=np.float32)
        props[:, 1:5], props[:, 5] = pb, rs.uniform(size=p)
        rgts = np.concatenate([gt[:, :4] * .5, gt[:, 4:]], 1).astype(np.float32)
        images.append({'name': 'r%02d' % i, 'info': f32(H, W, scale), 'gt': gt, 'det': det, 'props': props, 'rgts': rgts})
    return images, [(im['name'], im['gt']) for im in images], C


def record(name, images, records, C, cal, compute_recall, keep_num=100, recall_each=False):
    """run the reference and the restatement over one set -> the arrays of the fixture"""
    rows = [r for im in images for r in text_rows(im, C, keep_num)]
    meta = meta_lines(records)
    gts = cal.parse_gts(meta, C)
    results = cal.parse_res(rows)
    empty = [c for c in range(1, C) if len(results[c]) == 0]
    if empty:
        try:
            cal.cal_mAP(cal.parse_gts(meta, C), results, C, 0.5)
            raise AssertionError("the reference was expected to raise for a class without rows")
        except ValueError:
            pass
    cal.np = _NumpyEmptyMax()
    try:
        with np.errstate(divide='ignore', invalid='ignore'):
            ap, max_recall = cal.cal_mAP(gts, results, C, 0.5)
    finally:
        cal.np = np
    index = {im['name']: i for i, im in enumerate(images)}
    res = np.asarray([[c, index[r[5]]] + r[:4] for c in range(1, C) for r in results[c]], dtype=np.int32).reshape(-1, 6)
    res_score = np.asarray([r[4] for c in range(1, C) for r in results[c]], dtype=np.float64)
    is_det = []
    for im in images:
        flags = np.zeros(len(im['gt']), dtype=np.uint8)
        if im.get('in_meta', True):
            for c in range(1, C):
                at = np.nonzero(im['gt'][:, 4] == c)[0]
                flags[at] = np.asarray(gts[im['name']]['is_det'][c]).astype(np.uint8)
        is_det.append(flags)
    sum_gt = np.asarray(gts['num']).astype(np.int64)
    # ---- the restatement must give the reference's numbers before its per-row flags are recorded
    mine = vnp.evaluate(images, C, sum_gt=sum_gt, keep_num=keep_num)
    assert np.array_equal(mine['ap'], ap, equal_nan=True) and np.array_equal(mine['max_recall'], max_recall, equal_nan=True), (name, mine['ap'], ap)
    assert mine['ap'].tobytes() == np.asarray(ap).tobytes() or np.isnan(ap).any()
    for c in range(1, C):
        assert sum(int(e['tp'][e['cls'] == c].sum()) for e in mine['per_image']) == sum(int(f[im['gt'][:, 4] == c].sum()) for f, im in zip(is_det, images))
    assert all(np.array_equal(e['claimed'], f) for e, f in zip(mine['per_image'], is_det))
    out = {'C': np.int64(C), 'names': np.asarray([im['name'] for im in images]), 'info': np.stack([im['info'] for im in images]),
           'det': np.concatenate([im['det'] for im in images]), 'det_counts': np.asarray([len(im['det']) for im in images], dtype=np.int32),
           'gt': np.concatenate([im['gt'] for im in images]).astype(np.int32), 'gt_counts': np.asarray([len(im['gt']) for im in images], dtype=np.int32),
           'in_meta': np.asarray([im.get('in_meta', True) for im in images], dtype=np.uint8), 'sum_gt': sum_gt,
           'res': res, 'res_score': res_score, 'ap': np.asarray(ap), 'max_recall': np.asarray(max_recall), 'mAP': np.mean(ap[1:]),
           'is_det': np.concatenate(is_det), 'tp': np.concatenate([e['tp'] for e in mine['per_image']]).astype(np.uint8),
           'match': np.concatenate([e['match'] for e in mine['per_image']]).astype(np.int32)}
    if 'props' in images[0]:
        rc = ng = 0
        each = []
        for im in images:
            r, g = compute_recall(im['props'][:, 1:5], im['rgts'])
            rc, ng = rc + int(r), ng + int(g)
            each.append((int(r), int(g)))
        assert (mine['rpn_recalled'], mine['rpn_gts']) == (rc, ng), (mine['rpn_recalled'], rc)
        out.update({'props': np.concatenate([im['props'] for im in images]), 'prop_counts': np.asarray([len(im['props']) for im in images], dtype=np.int32),
                    'rgts': np.concatenate([im['rgts'] for im in images]), 'rgt_counts': np.asarray([len(im['rgts']) for im in images], dtype=np.int32),
                    'recalled': np.int64(rc), 'rpn_gts': np.int64(ng)})
        if recall_each:                                                       # compute_recall's answer image by image too
            out['recalled_each'] = np.asarray(each, dtype=np.int32).reshape(-1, 2)
    return {name + '_' + k: v for k, v in out.items()}, mine


def main():
    if len(sys.argv) > 1:
        os.environ["SCDA_REFERENCE"] = sys.argv[1]
    import ref_harness
    cal = load_cal_map(ref_harness.REF)
    compute_recall = ref_harness.import_reference().bbox_helper.compute_recall
    out = {}
    # ---- rules
    images, records, C = rules_set()
    z, mine = record('rules', images, records, C, cal, compute_recall)
    out.update(z)
    per = {im['name']: e for im, e in zip(images, mine['per_image'])}
    tp = lambda n: per[n]['tp'].tolist()                                      # noqa: E731
    assert tp('a_half')[:4] == [1, 0, 0, 1] and not per['a_half']['kept'][4:].any()          # IoU 100 / 200; touching; one pixel wide; classes 0, 5, 7
    assert vnp.best_iou([0, 0, 9, 9], [[0, 0, 9, 19]]) == (0.5, 0) and vnp.best_iou([60, 50, 70, 60], [[50, 50, 60, 60]]) == (-1, -1)
    assert tp('b_claimed') == [1, 0, 1, 1, 0] and per['b_claimed']['match'].tolist() == [0, -1, 1, 2, -1]
    assert vnp.best_iou([10, 10, 49, 51], [[10, 10, 49, 49], [10, 10, 49, 69]])[1] == 0 and vnp.best_iou([10, 10, 49, 51], [[10, 10, 49, 69]])[0] >= .5
    assert per['c_trunc']['box'][0].tolist() == [0, 0, 9, 9] and tp('c_trunc')[0] == 1 and per['c_trunc']['box'][1].tolist() == [10, 30, 40, 60]
    assert per['d_clip']['box'].tolist() == [[300, 20, 398, 100], [100, 0, 140, 198]] and tp('d_clip') == [1, 1]
    x, k = scale13_coordinate()
    assert per['e_scale13']['box'][0, 2] == k and int(float(x) / float(np.float32(1.3))) == k - 1
    assert sorted(float(s) for s in np.unique(out['rules_info'][:, 2])) == [.5, 1.0, float(np.float32(1.3))]
    assert tp('f_ties') == [1, 0, 0] and tp('g_ties') == [0, 1]               # equal scores: row order; f's rows before g's in class 1
    h = per['h_130']
    assert len(h['tp']) == 130 and (h['rank'] < 100).sum() == 100
    cut = np.nonzero(images[7]['det'][:, 5] == np.float32(.3))[0]
    assert len(cut) == 10 and h['rank'][cut].tolist() == list(range(98, 108)) and not h['tp'][cut].any()
    assert h['kept'][cut].tolist() == [True, True] + [False] * 8 and not per['h_130']['claimed'][0]
    assert vnp.best_iou(h['box'][cut[2]], [[100, 50, 139, 89]]) == (1.0, 0)     # the third tied row would have been a true positive
    assert (images[7]['det'][h['rank'] < 100, 6] == 6).sum() > 0              # rows of a class that is never written use up places
    assert out['rules_gt_counts'][8] == 0 and out['rules_det_counts'][9] == 0 and out['rules_in_meta'][10] == 0
    assert out['rules_sum_gt'][1] == sum(int((im['gt'][:, 4] == 1).sum()) for im in images) + 2                 # never_added counts
    rows_of = [int((out['rules_res'][:, 0] == c).sum()) for c in range(C)]
    assert rows_of[4] == 0 and out['rules_sum_gt'][4] > 0 and out['rules_ap'][4] == 0                           # ground truths, no rows
    assert rows_of[2] > 1 and out['rules_sum_gt'][2] > 0 and out['rules_ap'][2] == 0 and out['rules_max_recall'][2] == 0    # all false positives
    assert rows_of[3] == 1 and out['rules_ap'][3] > 0                                                         # a single row
    assert per['w63']['match'].tolist() == [62, 0] and per['w64']['match'].tolist() == [63, -1]
    assert per['w65']['match'].tolist() == [-1, 65, 64] and tp('w65') == [0, 1, 1]      # the tie 63 / 64 (rows 64 / 65): the first; then it is claimed
    assert vnp.best_iou([345, 100, 364, 119], [[340, 100, 359, 119], [350, 100, 369, 119]]) == (0.6, 0)
    # ---- nan
    images, records, C = nan_set()
    z, mine = record('nan', images, records, C, cal, compute_recall)
    out.update(z)
    assert np.isnan(out['nan_ap'][2]) and np.isnan(out['nan_max_recall'][2]) and np.isfinite(out['nan_ap'][1]) and np.isnan(out['nan_mAP'])
    # ---- random
    images, records, C = random_set()
    z, mine = record('random', images, records, C, cal, compute_recall)
    out.update(z)
    assert np.all((out['random_ap'][1:] > 0) & (out['random_ap'][1:] < 1)) and np.isfinite(out['random_mAP'])
    assert 2048 < len(out['random_res']) and 0 < out['random_recalled'] < out['random_rpn_gts']
    sc = out['random_det'][:, 5]
    assert len(np.unique(sc)) < len(sc) and out['random_prop_counts'][5] == 0
    # ---- the edge sets of tests/eval_edge_cases.py (test_eval_edges_rules.py asserts the boundary each one crosses)
    for name in edges.MAP_SETS:
        images, records, C = edges.map_case(name)
        assert name + '_C' not in out
        z, mine = record(name, images, records, C, cal, compute_recall, keep_num=edges.MAP_CAPS[name]['keep_num'], recall_each=True)
        z[name + '_keep_num'] = np.int64(edges.MAP_CAPS[name]['keep_num'])
        out.update(z)
        print(name, "rows", len(z[name + '_res']), "mAP", z[name + '_mAP'])
    path = os.path.join(HERE, "voc_map_ref.npz")
    if os.path.exists(path):                                                  # regeneration must not move an array of the older sets
        with np.load(path) as old:
            for k in (k for k in old.files if not any(k.startswith(s + '_') for s in edges.MAP_SETS)):
                assert out[k].dtype == old[k].dtype and out[k].shape == old[k].shape and out[k].tobytes() == old[k].tobytes(), k
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "random mAP", out['random_mAP'], "rules ap", out['rules_ap'])


if __name__ == "__main__":
    main()
