"""The case table of the mask edge suite: inputs built from the constants of scda_amd/csrc/mask_rle.hip and mask_poly.hip (32-row
blocks, 32-column words, uint4 groups of 128 toggle bits, 256-entry scan rounds, 64-lane edge rounds), not from what masks look like.
tests/golden/make_golden_mask_edges.py records the reference's outputs for it (tests/golden/mask_edges_ref.npz),
tests/test_mask_edges_rules.py pins the numpy statements and the host fallback to them and asserts that every case still crosses the
boundary it was built for, tests/test_mask_edges_gpu.py runs the kernels.  The standard plane is 66 rows x 3 words: row blocks of 32,
32 and 2 rows and three word columns, the smallest plane with every block boundary, word boundary and tail.  numpy only."""
import numpy as np

import mask_rle_np as R

H, WD = 66, 3
W = 32 * WD


# ------------------------------------------------------------------------------------------------ planes
def pack(mask, H_=H, Wd=WD, dirty=False):
    """bool [h, w] -> uint32 [H_, Wd]; dirty: EVERY bit outside the h x w crop is set (such bits never count)"""
    full = np.full((H_, Wd * 32), 1 if dirty else 0, dtype=np.uint8)
    full[:mask.shape[0], :mask.shape[1]] = mask
    return np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(H_, Wd)


def ragged(arrays, dtype):
    """list of 1-d arrays -> (concatenation, first int32 [n + 1])"""
    first = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int32)
    flat = np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays]) if arrays else np.zeros(0, dtype)
    return flat.astype(dtype), first


def cut(flat, first, i):
    return flat[first[i]:first[i + 1]]


# ------------------------------------------------------------------------------------------------ 1a: the encoder
ENC_SIZES = ((66, 96), (65, 95), (64, 64), (33, 33), (32, 32), (32, 96), (31, 64), (2, 33), (1, 96), (66, 1), (1, 1))


def patterns(h, w, seed):
    """-> [(name, bool [h, w])]: the patterns that fit an h x w image"""
    z = lambda: np.zeros((h, w), dtype=bool)                                  # noqa: E731
    yy, xx = np.mgrid[:h, :w]
    out = [('empty', z()), ('full', ~z())]
    for name, y, x in (('first', 0, 0), ('last', h - 1, w - 1), ('bottom31', h - 1, 31), ('bottom32', h - 1, 32), ('top32', 0, 32)):
        if x < w:
            m = z(); m[y, x] = True; out.append((name, m))
    for name, cols in (('col31', (31,)), ('col32', (32,)), ('col31_32', (31, 32))):  # col31_32: ONE run across the word boundary
        if max(cols) < w:
            m = z(); m[:, list(cols)] = True; out.append((name, m))
    if h > 32:
        m = z(); m[31:33] = True; out.append(('rows31_32', m))                # the row-block boundary
    m = z(); m[h - 1] = True; out.append(('last_row', m))
    # the checkerboard of the column-major sequence (for an even h it is rows): EVERY pixel is a transition, column ends included
    out.append(('checker0', (xx * h + yy) % 2 == 1))                          # h * w runs
    out.append(('checker1', (xx * h + yy) % 2 == 0))                          # first pixel set: h * w + 1 runs
    out.append(('stripes', xx % 2 == 1))
    out.append(('random', np.random.RandomState(seed).rand(h, w) < 0.5))
    return out


def encoder_cases():
    """-> [{'name', 'h', 'w', 'mask'}]; every case is run as pack(mask) and as pack(mask, dirty=True)"""
    cases = []
    for i, (h, w) in enumerate(ENC_SIZES):
        for name, m in patterns(h, w, 100 + i):
            cases.append({'name': '%dx%d/%s' % (h, w, name), 'h': h, 'w': w, 'mask': m})
    return cases


def batch300():
    """300 planes of [3, 1] words for image_info of 100 rows (masks_per_image = 3) -> (bits uint32 [300, 3, 1], info f32 [100, 2]);
    the bits outside an image's size are random as well"""
    rng = np.random.RandomState(300)
    full = rng.rand(300, 3, 32) < 0.5
    info = np.stack([rng.randint(1, 4, 100), rng.randint(1, 33, 100)], 1).astype(np.float32)
    info[:4] = ((3, 32), (1, 1), (3, 1), (1, 32))
    return np.stack([pack(m, 3, 1) for m in full]), info


def wide_batch():
    """planes of 3 rows x 10 words: more than 256 columns, so that the column scan of a mask takes a second round of 256 and the
    second round starts from the first one's total -> (bits uint32 [4, 3, 10], sizes f32 [4, 2])"""
    rng = np.random.RandomState(320)
    full = rng.rand(4, 3, 320) < 0.5
    return np.stack([pack(m, 3, 10) for m in full]), np.array(((3, 320), (3, 300), (2, 289), (1, 257)), dtype=np.float32)


# ------------------------------------------------------------------------------------------------ 1b: the RoI hint
WINDOWS = ((0, 0, 31, 65), (32, 0, 63, 65), (64, 0, 95, 65), (31, 0, 32, 65), (10, 3, 40, 20), (0, 65, 95, 65), (-7, -3, 5, 70),
           (90, 0, 200, 65), (96, 0, 120, 65), (50, 10, 40, 30), (float('nan'), 0, 5, 5), (0, 0, 6e8, 5), (-3.5, 0, -1.2, 10),
           (31.9, 0.2, 63.99, 65.5))
HINT_IMAGES = ((66, 96), (66, 70), (40, 64))


def trunc(v):
    """float32 -> int as the paste truncates a RoI coordinate; None where it refuses (not finite or beyond +-5e8)"""
    v = np.float32(v)
    if not (v > np.float32(-5.0e8) and v < np.float32(5.0e8)):
        return None
    return int(v)


def window_mask(win, h, w, fill):
    """the mask the paste would leave for window (x1, y1, x2, y2) in an h x w image: set only inside the truncated window, all of it
    (fill None) or a seeded half of it (fill = seed); a dead window gives the all-zero plane"""
    m = np.zeros((h, w), dtype=bool)
    t = [trunc(v) for v in win]
    if any(v is None for v in t):
        return m
    x1, y1, x2, y2 = t
    if x2 - x1 + 1 <= 0 or y2 - y1 + 1 <= 0:
        return m
    xa, xb, ya, yb = max(x1, 0), min(x2 + 1, w), max(y1, 0), min(y2 + 1, h)
    if xa >= xb or ya >= yb:
        return m
    m[ya:yb, xa:xb] = True if fill is None else np.random.RandomState(fill).rand(yb - ya, xb - xa) < 0.5
    return m


def hint_cases():
    """-> [{'name', 'h', 'w', 'roi' f32 [5], 'mask'}]"""
    cases = []
    for (h, w) in HINT_IMAGES:
        for k, win in enumerate(WINDOWS):
            for fill in (None, 500 + k):
                cases.append({'name': '%dx%d/win%d/%s' % (h, w, k, 'full' if fill is None else 'random'), 'h': h, 'w': w,
                              'roi': np.array((0,) + tuple(win), dtype=np.float32), 'mask': window_mask(win, h, w, fill)})
    return cases


# ------------------------------------------------------------------------------------------------ 1c: six-character counts
LARGE = {'h': 4100, 'w': 4100, 'Wd': 129, 'ones': 16800000}                   # positions [0, ones) and ones + 1 are set


def large_mask():
    """bool [4100, 4100]: the column-major positions [0, 16 800 000) set, 16 800 000 clear, 16 800 001 set, the rest clear"""
    h, w, n = LARGE['h'], LARGE['w'], LARGE['ones']
    flat = np.zeros(h * w, dtype=bool)
    flat[:n] = True
    flat[n + 1] = True
    return flat.reshape(w, h).T


# ------------------------------------------------------------------------------------------------ 1d: mask IoU
IOU_SIZES = ((66, 96), (65, 95), (33, 64), (32, 32), (1, 96), (66, 1))


def _cols(h, w, a, b):
    m = np.zeros((h, w), dtype=bool)
    m[:, max(a, 0):min(b, w)] = True
    return m


def iou_masks(h, w, seed):
    """-> (names, dt bool [M, h, w], gt bool [N, h, w]), M = N + 2.  Column bands are clipped to the image (a band that does not fit is
    one more empty mask)."""
    z = np.zeros((h, w), dtype=bool)
    last = z.copy(); last[h - 1, w - 1] = True
    rng = np.random.RandomState(seed)
    both = [('empty', z), ('full', ~z), ('last', last), ('random', rng.rand(h, w) < 0.5),
            ('to31', _cols(h, w, 0, 32)), ('from31', _cols(h, w, 31, 41)),          # meet only in column 31
            ('to32', _cols(h, w, 20, 33)), ('from32', _cols(h, w, 32, w)),          # meet only in column 32
            ('to32b', _cols(h, w, 0, 33)), ('from31b', _cols(h, w, 31, w)),         # meet only across 31 | 32
            ('c30_31', _cols(h, w, 30, 32)), ('c32_33', _cols(h, w, 32, 34))]       # column-disjoint, neighbouring words
    if h >= 35 and w >= 33:
        # the run from (31, 31) wraps into column 32 and ends at (30, 32): rleToBbox gives rows 30..31, the two pixels (33..34, 31) of
        # the other mask lie below that box -- intersection 2, o = 0
        wrap = z.copy(); wrap[31:, 31] = True; wrap[:31, 32] = True
        two = z.copy(); two[33:35, 31] = True
        both += [('wrap', wrap), ('two', two)]
    extra = [('random2', rng.rand(h, w) < 0.1), ('first', np.roll(last.reshape(-1), 1).reshape(h, w))]
    names = [n for n, _ in both + extra]
    return names, np.stack([m for _, m in both + extra]), np.stack([m for _, m in both])


def iou_crowd(n):
    """iscrowd of the first call; the second call takes 1 - this"""
    return (np.arange(n) % 2).astype(np.uint8)


def iou_m70():
    """M = 70, N = 3 on 66 x 96: seeded rectangles -> (dt bool [70, 66, 96], gt bool [3, 66, 96], iscrowd uint8 [3])"""
    rng = np.random.RandomState(70)
    out = []
    for n in (70, 3):
        m = np.zeros((n, H, W), dtype=bool)
        for i in range(n):
            y, x = rng.randint(0, H), rng.randint(0, W)
            m[i, y:y + 1 + rng.randint(H), x:x + 1 + rng.randint(W)] = True
        out.append(m)
    out[1][2] = out[0][41]                                                    # one identical pair off the diagonal
    return out[0], out[1], np.array([0, 1, 0], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ 1e: annToMask
POLY_SIZES = ((32, 32), (64, 64), (4, 32), (1, 32), (33, 31), (1, 33), (1, 1), (66, 96), (65, 95))


def _split(total, k):
    """k runs that sum to total exactly (the remainder goes to the last)"""
    c = [total // k] * k
    c[-1] += total - sum(c)
    return c


def rles(h, w, seed):
    """-> [(name, counts list)]: the uncompressed RLEs of an h x w image; every sum is <= h * w"""
    n = h * w
    a = n // 5
    out = [('all', [n]), ('zero_all', [0, n]), ('even_exact', _split(n, 4)), ('odd_exact', _split(n, 5)), ('below', [n // 3, n // 3]),
           ('one_run', [n // 2]), ('zeros_inside', [a, 0, a, a, 0, 0, a])]
    rng = np.random.RandomState(seed)
    for m in (600, 1100):                       # more than one, and more than four, rounds of 256 runs
        c = rng.randint(1, 4, m).tolist()
        if sum(c) <= n:
            out.append(('runs%d' % m, c))
    return out


def _rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def polygons(h, w):
    """-> [(name, [float64 [k, 2]])]: the single-polygon cases of an h x w image"""
    return [('image', [_rect(0, 0, w, h)]), ('to_w', [_rect(w / 2.0, 0, w, h)]), ('to_w_1', [_rect(w / 2.0, 0, w - 1, h)]),
            ('left_above', [_rect(-30, -20, -5, -3)]), ('right_below', [_rect(w + 5, h + 3, w + 30, h + 20)]),
            ('diagonal', [np.array([[0, 0], [w, h], [0, h / 3.0]], dtype=np.float64)]),      # 66 x 96: an edge of 481 points
            ('one_vertex', [np.array([[w / 2.0, h / 2.0]])]), ('two_vertices', [np.array([[0.2, 0.1], [w - 0.3, h - 0.4]])])]


def poly_cases():
    """-> one entry per plane of the [n, 66, 3] batch, None for a plane that nothing maps to, else {'name', 'h', 'w', 'polygons':
    [float64 [k, 2]] (k = 0: an empty polygon slot), 'counts': uint32 or None, 'string': bytes or None (the compressed form of
    'counts', which then reaches the kernel through the host's string decode)}"""
    planes = [None]
    for i, (h, w) in enumerate(POLY_SIZES):
        tag = '%dx%d/' % (h, w)
        for name, c in rles(h, w, 700 + i):
            c = np.asarray(c, dtype=np.uint32)
            planes.append({'name': tag + 'rle/' + name, 'h': h, 'w': w, 'polygons': [], 'counts': c, 'string': None})
            planes.append({'name': tag + 'str/' + name, 'h': h, 'w': w, 'polygons': [], 'counts': c, 'string': R.to_string(c)})
        planes.append(None)
        for name, p in polygons(h, w):
            planes.append({'name': tag + 'poly/' + name, 'h': h, 'w': w, 'polygons': p, 'counts': None, 'string': None})
        tri = np.array([[1.5, 0.5], [w - 0.5, h * 0.4], [w * 0.3, h - 0.2]])
        planes.append({'name': tag + 'empty_slot', 'h': h, 'w': w, 'polygons': [_rect(0.4, 0.4, w * 0.6, h * 0.5), np.zeros((0, 2)), tri],
                       'counts': None, 'string': None})
        planes.append({'name': tag + 'union', 'h': h, 'w': w, 'counts': np.asarray(_split(h * w, 6), dtype=np.uint32), 'string': None,
                       'polygons': [_rect(0.4, 0.4, w * 0.6, h * 0.5), tri, _rect(w * 0.5, h * 0.25, w + 3, h * 0.8)]})
    planes.append(None)
    return planes


BIG = {'H': 363, 'Wd': 12, 'h': 363, 'w': 365}                                # 132 495 pixels: a second round of 256 x 128 toggle bits


def poly_big_cases():
    """-> the planes of a [4, 363, 12] batch whose fills run across bit 131 072 of the toggle plane, where the parity scan's second
    round starts from the parity of the first"""
    h, w = BIG['h'], BIG['w']
    c = np.array([5, 131070, 3, 1000, 20], dtype=np.uint32)                   # ones from 5 to 131 075, odd run count
    case = lambda name, polygons, counts, string: {'name': 'big/' + name, 'h': h, 'w': w, 'polygons': polygons, 'counts': counts,  # noqa: E731
                                                   'string': string}
    return [case('rle', [], c, None), None, case('str', [], c, R.to_string(c)), case('poly', [_rect(10, 10, w - 2, h - 3)], None, None)]


def flat_annotations(planes):
    """the flat arrays of scda_mask_frpoly_hip for one shape list per plane -> dict of numpy arrays"""
    xy, poly_first, poly_plane, counts, rle_first, rle_plane, sizes = [np.zeros((0, 2))], [0], [], [np.zeros(0, np.uint32)], [0], [], []
    for n, c in enumerate(planes):
        sizes.append((5, 7) if c is None else (c['h'], c['w']))
        if c is None:
            continue
        for p in c['polygons']:
            xy.append(np.asarray(p, dtype=np.float64).reshape(-1, 2)); poly_first.append(poly_first[-1] + len(p)); poly_plane.append(n)
        if c['counts'] is not None:
            counts.append(np.asarray(c['counts'], dtype=np.uint32)); rle_first.append(rle_first[-1] + len(c['counts'])); rle_plane.append(n)
    i32 = lambda a: np.asarray(a, dtype=np.int32)                             # noqa: E731
    return {'xy': np.concatenate(xy), 'poly_first': i32(poly_first), 'poly_plane': i32(poly_plane), 'rle_counts': np.concatenate(counts),
            'rle_first': i32(rle_first), 'rle_plane': i32(rle_plane), 'sizes': i32(sizes).reshape(-1, 2)}


# ------------------------------------------------------------------------------------------------ the recorded outputs
_FIXTURE = {}


def fixture(golden_dir):
    """tests/golden/mask_edges_ref.npz as a dict of arrays (read once)"""
    import os
    if golden_dir not in _FIXTURE:
        with np.load(os.path.join(golden_dir, "mask_edges_ref.npz")) as z:
            _FIXTURE[golden_dir] = {k: z[k] for k in z.files}
    return _FIXTURE[golden_dir]


def recorded(g, prefix, i):
    """case i of an encoder group as the reference recorded it, in the form of mask_rle_np.statement"""
    counts = cut(g[prefix + '_counts'], g[prefix + '_first'], i)
    return {'n_runs': len(counts), 'counts': counts, 'chars': cut(g[prefix + '_chars'], g[prefix + '_cfirst'], i).tobytes(),
            'area': int(g[prefix + '_area'][i]), 'bbox': [int(v) for v in g[prefix + '_bbox'][i]]}
