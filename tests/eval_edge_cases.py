"""Seeded builders of the evaluators' structural edge cases: inputs whose shapes come from the constants of scda_amd/csrc/coco_eval.hip,
map_eval.hip, radix_sort.h and the primitives they share in eval_prims.h (wave and block rounds, the LDS stage, the 32-detection flush,
the capacities, the parameter limits, the sort keys, the 256-row scan rounds), not from what data looks like.  tests/golden/make_golden_coco_eval.py and make_golden_voc_map.py
record the reference's outputs for them next to the older sets; tests/test_eval_edges_rules.py asserts that every case still crosses
the boundary it was built for and tests/test_eval_edges_gpu.py runs the kernels over them.  Boxes sit on an integer grid (the recorded
arrays compress, and equal IoUs are exact).  Nothing here depends on a GPU."""
import numpy as np

import coco_eval_np as cnp

# ------------------------------------------------------------------------------------------------ COCO
COCO_SETS = ('waves', 'capacity', 'limits', 'limits3', 'sortkeys', 'prrounds')
COCO_CAPS = {'waves': (400, 224), 'capacity': (1024, 1024), 'limits': (40, 24), 'limits3': (40, 24), 'sortkeys': (16, 8),
             'prrounds': (272, 32)}            # the evaluator's (detection slots, ground-truth slots) per image


def _coco_image(image_id, dets, gts, rs=None):
    """dets [n, 6] = (x1, y1, x2, y2, score, cat), gts [g, 7] = (x, y, w, h, iscrowd, cat, area), both shuffled when rs is given"""
    d = np.asarray(dets, dtype=np.float64).reshape(-1, 6)
    g = np.asarray(gts, dtype=np.float64).reshape(-1, 7)
    if rs is not None:
        d, g = d[rs.permutation(len(d))], g[rs.permutation(len(g))]
    return {'image_id': int(image_id), 'dt_corners': d[:, :4].astype(np.float32), 'dt_score': d[:, 4].astype(np.float32),
            'dt_cat': d[:, 5].astype(np.int32), 'gt_xywh': g[:, :4].copy(), 'gt_area': g[:, 6].copy(),
            'gt_iscrowd': g[:, 4].astype(np.uint8), 'gt_cat': g[:, 5].astype(np.int32)}


def _cluster(rs, cat, n_gt, n_det, crowds=0.1, span=(400, 300)):
    """n_gt ground truths of one category with integer boxes that overlap each other, n_det detections jittered from them (anywhere
    when there is no ground truth); scores in hundredths, so that they tie"""
    w, h = rs.randint(6, 140, n_gt), rs.randint(6, 140, n_gt)
    x, y = rs.randint(0, span[0], n_gt), rs.randint(0, span[1], n_gt)
    crowd = (rs.rand(n_gt) < crowds).astype(np.float64)
    gts = np.stack([x, y, w, h, crowd, np.full(n_gt, cat), w * h * rs.choice([0.5, 1.0], n_gt)], 1).astype(np.float64).reshape(-1, 7)
    if n_gt:
        src = rs.randint(0, n_gt, n_det)
        q = np.maximum(1, np.stack([w, h, w, h], 1)[src] // rs.choice([4, 8, 32], n_det)[:, None])
        j = np.floor(rs.uniform(-1, 1, (n_det, 4)) * (q + 1)).astype(np.int64)
        x1, y1 = x[src] + j[:, 0], y[src] + j[:, 1]
        x2, y2 = x1 + w[src] + j[:, 2], y1 + h[src] + j[:, 3]
    else:
        x1, y1 = rs.randint(0, span[0], n_det), rs.randint(0, span[1], n_det)
        x2, y2 = x1 + rs.randint(6, 140, n_det), y1 + rs.randint(6, 140, n_det)
    dets = np.stack([x1, y1, x2, y2, rs.randint(5, 101, n_det) / 100.0, np.full(n_det, cat)], 1).astype(np.float64).reshape(-1, 6)
    return dets, gts


def _join(rs, image_id, clusters):
    return _coco_image(image_id, np.concatenate([c[0] for c in clusters]), np.concatenate([c[1] for c in clusters]), rs)


def _waves():
    """match_kernel's rounds: 64 / 65 ground truths (one wave round of wave_compact, two claim words, and one more), 128 / 129 detections
    (kMatchThreads), more than 100 (the tail loop), Gc * Dm = 2048 (staged) beside 64 x 33 (not staged), Dm = 32, 33, 64 and 0"""
    rs = np.random.RandomState(6401)
    big = _join(rs, 11, [_cluster(rs, 1, 64, 32), _cluster(rs, 2, 64, 33), _cluster(rs, 3, 65, 64), _cluster(rs, 4, 5, 0),
                         _cluster(rs, 5, 6, 128), _cluster(rs, 6, 6, 129)])
    small = _join(rs, 4, [_cluster(rs, 1, 3, 5), _cluster(rs, 6, 2, 4)])
    return {'images': [big, small], 'K': 6, 'params': cnp.default_params()}


def _capacity():
    """D = G = 1024: 1024 live detections of one category in one image; 1000 ground truths of a category in another (all 32 claim
    words, list positions >= 512, crowds up to the last ones) whose other categories stay small; an image without detections and one
    without ground truth.  n_images * D is a multiple of kSortTile = 1024"""
    rs = np.random.RandomState(1024)
    full = _join(rs, 5, [_cluster(rs, 1, 3, 1024)])
    dets, gts = _cluster(rs, 2, 1000, 40, crowds=0.0)
    gts[600::5, 4] = 1                                                        # 80 crowds; the shuffle spreads them up to the last positions
    crowded = _join(rs, 4, [(dets, gts), _cluster(rs, 3, 24, 4)])
    return {'images': [full, crowded, _join(rs, 3, [_cluster(rs, 1, 5, 0)]), _join(rs, 2, [_cluster(rs, 3, 0, 6)])],
            'K': 3, 'params': cnp.default_params()}


def _limits(max_dets):
    """the documented parameter limits: 16 IoU thresholds (1.0 among them, .5 and .75 not), 8 area ranges, 128 recall thresholds and
    the given maxDets; one detection is its ground truth's box (IoU 1.0, matched at the threshold clamped to 1 - 1e-10)"""
    rs = np.random.RandomState(168)
    images = []
    for i in range(3):
        d1, g1 = _cluster(rs, 1, 12, 34)
        g1[0, 4] = 0
        d1[0] = (g1[0, 0], g1[0, 1], g1[0, 0] + g1[0, 2], g1[0, 1] + g1[0, 3], 1.0, 1)
        images.append(_join(rs, 30 - 7 * i, [(d1, g1), _cluster(rs, 2, 8, 5)]))
    area = np.concatenate([cnp.default_params()['area_rng'], [[0, 400], [400, 4000], [4000, 1e10], [1e10, 2e10]]]).astype(np.float64)
    params = {'iou_thrs': np.linspace(.3, 1.0, 16), 'rec_thrs': np.linspace(.0, 1.0, 128), 'max_dets': list(max_dets), 'area_rng': area}
    return {'images': images, 'K': 2, 'params': params}


def _sortkeys():
    """the sort keys: negative scores, +0.0, -0.0 and a denormal; equal scores over three images that are added in descending id order;
    a negative image id and one >= 2^24; K = 255 with rows in categories 1 and 255; n_images * D < 64"""
    rs = np.random.RandomState(255)
    pool = [0.5, -0.25, 0.0, 1e-40, 0.5, -1.5, 0.75, -0.25]
    images = []
    for i, image_id in enumerate((2 ** 24 + 5, 7, -3)):
        clusters = []
        for cat, n_gt, n_det in ((1, 3, 8), (255, 2, 6)):
            dets, gts = _cluster(rs, cat, n_gt, n_det, crowds=0.0)
            for j in range(n_det):
                g = gts[(i + j) % n_gt]
                hit = (i + j // 2) % 2 == 0                                   # every other one is a ground truth's box, the rest far off
                dets[j, :4] = (g[0], g[1], g[0] + g[2], g[1] + g[3]) if hit else (900 + 3 * j, 700, 930 + 3 * j, 760)
                dets[j, 4] = pool[j]
            if i == 1:
                dets[dets[:, 4] == 0.0, 4] = -0.0
            clusters.append((dets, gts))
        images.append(_join(rs, image_id, clusters))
    params = dict(cnp.default_params(), iou_thrs=np.array([.5, .75]), rec_thrs=np.linspace(.0, 1.0, 11))
    return {'images': images, 'K': 255, 'params': params}


PR_ROWS = {1: (100, 100, 56, 0, 0, 0), 2: (0, 57, 0, 100, 100, 0), 3: (110,) * 6}          # detections per (category, image)


def _prrounds():
    """pr_kernel's 256-row rounds: categories with exactly 256, 257 and 600 participating rows (rank < 100) over six images; maxDets 1
    and 10 then drop rows in the middle of every round"""
    rs = np.random.RandomState(257)
    images = [_join(rs, 100 + 3 * i, [_cluster(rs, k, 10, PR_ROWS[k][i]) for k in (1, 2, 3)]) for i in range(6)]
    return {'images': images, 'K': 3, 'params': cnp.default_params()}


def coco_case(name):
    """-> {'images', 'K', 'params', 'D', 'G'} (D, G: the evaluator's per-image capacities, COCO_CAPS)"""
    case = {'waves': _waves, 'capacity': _capacity, 'limits': lambda: _limits([1, 5, 20, 100]), 'limits3': lambda: _limits([2, 7, 30]),
            'sortkeys': _sortkeys, 'prrounds': _prrounds}[name]()
    case['D'], case['G'] = COCO_CAPS[name]
    return case


def load_coco_set(z, name):
    """one edge set of coco_eval_ref.npz -> (images, K, params).  The IoU matrices are not stored: cnp.bb_iou, held bit-equal to the
    reference's bbIou by test_coco_eval_rules.py, recomputes them"""
    view = {k: v for k, v in z.items() if k.startswith(name + '_')}
    dc, gc = z[name + '_dt_counts'], z[name + '_gt_counts']
    do, go = np.concatenate([[0], np.cumsum(dc)]), np.concatenate([[0], np.cumsum(gc)])
    xywh = cnp.xywh_from_corners(z[name + '_dt_corners'])
    view[name + '_iou'] = np.concatenate([np.zeros(0)] + [
        cnp.bb_iou(xywh[do[i]:do[i + 1]], z[name + '_gt_boxes'][go[i]:go[i + 1]], z[name + '_gt_iscrowd'][go[i]:go[i + 1]]).reshape(-1)
        for i in range(len(dc))])
    images, K, params = cnp.load_set(view, name)
    params.update(iou_thrs=z[name + '_iou_thrs'], rec_thrs=z[name + '_rec_thrs'], max_dets=[int(m) for m in z[name + '_max_dets']])
    return images, K, params


# ------------------------------------------------------------------------------------------------ Cityscapes mAP
MAP_SETS = ('cap', 'keep100', 'match', 'recall')
MAP_CAPS = {'cap': dict(D=1024, G=32, keep_num=1024), 'keep100': dict(D=1024, G=32, keep_num=100),
            'match': dict(D=320, G=1024, keep_num=320), 'recall': dict(D=4, G=4, keep_num=4, P=256, RG=16)}
CAP_CLASS_ROWS = {1: 256, 2: 257, 3: 1000, 4: 8, 5: 6, 0: 5, 9: 5}           # rows per class over the three images (0 and 9: never written)


def _det_rows(rows):
    out = np.zeros((len(rows), 7), dtype=np.float32)
    if len(rows):
        out[:, 1:] = np.asarray(rows, dtype=np.float64)
    return out


def _gt_rows(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 5)


def _map_cap():
    """map_rows_kernel's rounds and map_pr_kernel's: images with 256, 257 and 1024 = D live detections; with keep_num = D the classes
    have exactly 256, 257 and 1000 rows; class 4's rows are all false positives, class 5 has rows and no ground truth (NaN); scores
    negative, +0.0, -0.0, tied inside and across the images.  The same images with keep_num = 100 are the set 'keep100'"""
    rs = np.random.RandomState(1537)
    cls = rs.permutation(np.concatenate([np.full(n, c) for c, n in CAP_CLASS_ROWS.items()]))
    info = np.asarray([600, 800, 1.0], dtype=np.float32)
    images, at = [], 0
    for name, n in (('c256', 256), ('c257', 257), ('c1024', 1024)):
        gts = []
        for c, g in ((1, 8), (2, 8), (3, 12)):
            x, y = rs.randint(0, 600, g), rs.randint(0, 400, g)
            gts += [(x[j], y[j], x[j] + rs.randint(10, 120), y[j] + rs.randint(10, 120), c) for j in range(g)]
        gts += [(700, 500, 780, 580, 4), (720, 520, 790, 590, 4)]             # class 4: out of its detections' reach
        gts = _gt_rows(gts)[rs.permutation(len(gts))]
        rows = []
        for c in cls[at:at + n]:
            mine = gts[gts[:, 4] == c]
            if c in (1, 2, 3):
                g = mine[rs.randint(len(mine))]
                box = g[:4] + rs.randint(-6, 7, 4) + rs.choice([0.0, 0.25, 0.5], 4)             # fractions: the truncation counts
            else:
                x, y = rs.randint(-5, 300), rs.randint(-5, 300)              # a few start left of / above the image: the clip
                box = (x, y, x + rs.randint(10, 120), y + rs.randint(10, 120))
            score = 0.99 if c in (4, 5) else rs.randint(-50, 101) / 100.0     # classes 4 and 5 stay among the best 100 of their image
            rows.append(tuple(box) + (score, c))
        det = _det_rows(rows)
        zero = np.flatnonzero(det[:, 5] == 0)
        det[zero[::2], 5] = -0.0
        images.append({'name': name, 'info': info, 'gt': gts, 'det': det})
        at += n
    return images, [(im['name'], im['gt']) for im in images], 6


def match_gt(k):
    """the k-th class-7 ground truth of the image 'g1000': 20 x 10 boxes, 40 in a row at a pitch of 12, so that neighbours overlap"""
    x, y = 12 * (k % 40), 25 * (k // 40)
    return [x, y, x + 19, y + 9]


MATCH_DUPS = (130, 900)                        # the boxes at j, j + 1 and j + 64 of 'g1000' are one box
MATCH_STRADDLE = (5, 63, 127, 511, 700, 998)   # a detection halfway between the boxes j and j + 1: the same IoU 14 / 26 with both


def _map_match():
    """map_match_kernel's rounds and the class limit: C = 256 with rows and ground truths in classes 1 and 255 and a row in every class;
    a class with exactly 64, 65 and 1000 ground truths; one box at the indices j, j + 1 and j + 64 (the first is claimed, the next
    detection with that box finds it taken); detections halfway between two ground truths (equal IoU in neighbouring lanes, across the
    wave round at 63 | 64); detections that overlap nothing strictly"""
    rs = np.random.RandomState(64065)
    info = np.asarray([700, 900, 1.0], dtype=np.float32)
    grid = lambda j, c: [20 * (j % 16), 20 * (j // 16), 20 * (j % 16) + 9, 20 * (j // 16) + 9, c]            # noqa: E731
    images = []
    # every class has a row; classes 1 and 255 a true positive
    rows = [(3 * c, 2 * c, 3 * c + 30, 2 * c + 20, rs.randint(5, 100) / 100.0, c) for c in range(1, 256)]
    images.append({'name': 'all', 'info': info, 'gt': _gt_rows([(3, 2, 33, 22, 1), (765, 510, 795, 530, 255), (100, 100, 150, 150, 128)]),
                   'det': _det_rows([rows[i] for i in rs.permutation(255)])})
    # exactly 64 of class 1: the last one, the first one, a box that overlaps nothing, a box that only touches
    images.append({'name': 'g64', 'info': info, 'gt': _gt_rows([grid(j, 1) for j in range(64)] + [(400, 300, 440, 340, 255)] * 3),
                   'det': _det_rows([tuple(grid(63, 1)[:4]) + (.9, 1), tuple(grid(0, 1)[:4]) + (.8, 1), (600, 600, 620, 620, .7, 1),
                                     (9, 0, 20, 9, .6, 1), (400, 300, 440, 340, .5, 255), (400, 300, 440, 340, .5, 255)])})
    # exactly 65 of class 255 between rows of class 3; the boxes at the class's indices 63 and 64 are one box
    g65 = [grid(j, 255) for j in range(65)]
    g65[64][:4] = g65[63][:4]
    mixed, k = [], 0
    for j in range(75):
        if j % 7 == 3 and j // 7 < 10:
            mixed.append([500 + 10 * (j // 7), 400, 540 + 10 * (j // 7), 440, 3])
        else:
            mixed.append(g65[k]); k += 1
    assert k == 65
    images.append({'name': 'g65', 'info': info, 'gt': _gt_rows(mixed),
                   'det': _det_rows([tuple(g65[63][:4]) + (.9, 255), tuple(g65[63][:4]) + (.8, 255), tuple(g65[64][:4]) + (.7, 255),
                                     tuple(g65[10][:4]) + (.95, 255), (505, 400, 545, 440, .6, 3)])})
    # 1000 of class 7, 24 of classes 1 and 255 between them
    g7 = [match_gt(k) + [7] for k in range(1000)]
    for j in MATCH_DUPS:
        g7[j + 1][:4] = g7[j + 64][:4] = g7[j][:4]
    others = {int(p): [600 + (i % 6) * 40, 100 + (i // 6) * 50, 630 + (i % 6) * 40, 140 + (i // 6) * 50, 1 if i % 2 else 255]
              for i, p in enumerate(sorted(rs.choice(1024, 24, replace=False)))}
    gts, k = [], 0
    for p in range(1024):
        if p in others:
            gts.append(others[p])
        else:
            gts.append(g7[k]); k += 1
    assert k == 1000
    rows, s = [], 0.99
    for j in MATCH_DUPS:
        for _ in range(3):
            rows.append(tuple(g7[j][:4]) + (s, 7)); s -= 0.01
    for j in MATCH_STRADDLE:
        b = match_gt(j)
        rows.append((b[0] + 6, b[1], b[2] + 6, b[3], s, 7)); s -= 0.01
    for k in rs.choice(1000, 24, replace=False):
        b = match_gt(int(k))
        rows.append((b[0] + rs.randint(-3, 4), b[1] + rs.randint(-2, 3), b[2] + rs.randint(-3, 4), b[3] + rs.randint(-2, 3), rs.randint(5, 60) / 100.0, 7))
    rows += [(850, 650, 880, 690, .5, 7), (600, 100, 630, 140, .4, 255), (640, 100, 670, 140, .4, 1)]
    images.append({'name': 'g1000', 'info': info, 'gt': _gt_rows(gts), 'det': _det_rows([rows[i] for i in rs.permutation(len(rows))])})
    return images, [(im['name'], im['gt']) for im in images], 256


RECALL_SHAPES = ((0, 4), (64, 1), (65, 5), (200, 9), (64, 0))                # (live proposals, ground-truth rows) per image


def _map_recall():
    """map_recall_kernel: 0, 64, 65 and 200 live proposals of P = 256; 0, 1, 4, 5 and 9 ground-truth rows (four waves, one row each a
    round); a row whose only overlapping proposal sits at index 64 and one at index 150; an overlap of exactly 0.5 that must not count"""
    rs = np.random.RandomState(465)
    info = np.asarray([512, 1024, 1.0], dtype=np.float32)
    images = []
    for i, (p, r) in enumerate(RECALL_SHAPES):
        x, y = rs.randint(0, 400, r).astype(np.float64), rs.randint(0, 300, r).astype(np.float64)
        rgts = np.stack([x, y, x + rs.randint(20, 90, r), y + rs.randint(20, 90, r), np.ones(r)], 1).reshape(-1, 5)
        props = np.zeros((p, 6))
        if p:
            src = rgts[rs.randint(0, max(r, 1), p) % max(r, 1), :4] if r else np.tile([10.0, 10.0, 50.0, 50.0], (p, 1))
            props[:, 1:5] = src + rs.randint(-12, 13, (p, 4))
            props[:, 5] = rs.uniform(size=p)
        if (p, r) == (65, 5):                                                 # row 0: alone at the far corner, found by proposal 64 only
            rgts[0, :4] = (900, 400, 960, 460)
            props[:, 1:5] = np.minimum(props[:, 1:5], 600)
            props[64, 1:5] = (902, 401, 961, 462)
        if (p, r) == (200, 9):
            rgts[8, :4] = (900, 400, 960, 460)
            props[:, 1:5] = np.minimum(props[:, 1:5], 600)
            props[150, 1:5] = (899, 398, 958, 460)
            rgts[4, :4] = (800, 10, 802, 11)                                  # overlap with (800, 10, 801, 11): 1 / (2 + 1 - 1) = 0.5
            props[7, 1:5] = (800, 10, 801, 11)
        images.append({'name': 'p%d' % i, 'info': info, 'gt': _gt_rows([(10, 10, 50, 50, 1)]), 'det': _det_rows([(10, 10, 50, 50, .9, 1)]),
                       'props': props.astype(np.float32), 'rgts': rgts.astype(np.float32)})
    return images, [(im['name'], im['gt']) for im in images], 2


def map_case(name):
    """-> (images to add, meta records, C); MAP_CAPS[name] holds the evaluator's capacities and keep_num"""
    return {'cap': _map_cap, 'keep100': _map_cap, 'match': _map_match, 'recall': _map_recall}[name]()
