"""Generates tests/golden/mask_poly_ref.npz with the REFERENCE's polygon / RLE code: datasets/pycocotools/common/maskApi.c is compiled
UNMODIFIED with the system C compiler into a temporary directory (gcc -O2 -fPIC -shared -std=c99 -I<common>, as make_golden_mask_rle.py
does) and rleFrPoly, rleMerge (intersect = 0), rleFrString, rleToString, rleDecode and rleEncode are called through ctypes -- the chain
of COCO.annToMask.  Run in the build container:
    python tests/golden/make_golden_mask_poly.py [path of the reference checkout]

Neither the C file nor the library is kept.  The file holds inputs and recorded outputs only; a result is stored as the run counts of
the decoded mask (rleEncode of rleDecode), never as a dense plane.  One case = one annotation of one image size:
  a  ~200 seeded random polygons, 1 x 1 .. 40 x 70, 1..8 vertices, in five styles: inside the image, leaving it on every side, on
     integers, on half pixels, with repeated coordinates and inserted duplicate vertices
  b  the full-image square on 10 x 10          c  a polygon far outside on all sides, 7 x 9
  d  one- and two-vertex polygons and a zero-width polygon (empty masks)
  e  polygons with a duplicated vertex whose reference mask DIFFERS from the polygon without it (a seeded search), and their twins
  f  5 x 33 and 37 x 70 (h * w no multiple of 32): polygons with run boundaries exactly on column ends
  g  annotations of 2..4 overlapping and disjoint polygons (rleMerge)
  h  uncompressed RLEs: first run 0, last run ending at h * w, counts summing to less than h * w
  i  the same as compressed strings; one 800 x 1344 string whose differences need 1..5 characters, negative ones included
  j  two 800 x 1344 annotations: an ellipse of 64 vertices; three polygons, one with an image-diagonal edge
Arrays (n cases): group U1 [n], size int32 [n, 2], big uint8 [n] (800 x 1344 cases), poly_first int32 [n + 1] (a case's polygons),
vert_first int32 [polygons + 1] and xy float64 [vertices, 2]; kind uint8 [n] (0 polygons, 1 uncompressed RLE, 2 compressed string),
rle_first int32 [n + 1] into rle_counts uint32 (kind 1: the input; kind 2: what rleFrString gives), str_first int32 [n + 1] into
str_bytes uint8 (kind 2: the input); out_first int32 [n + 1] into out_counts uint32 (the decoded mask's runs), area uint32 [n]
(rleArea), frpoly_first int32 [n + 1] into frpoly_counts uint32 (single-polygon cases: rleFrPoly's own counts)."""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_mask_rle import RLE, load_reference   # noqa: E402


def counts_of(r):
    return np.array([r.cnts[i] for i in range(r.m)], dtype=np.uint32)


def make_rle(counts, h, w):
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    r = RLE(h, w, len(c), c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)))
    r._keep = c
    return r


def fr_poly(lib, xy, h, w):
    a = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
    r = RLE()
    lib.rleFrPoly(ctypes.byref(r), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(len(a) // 2), ctypes.c_ulong(h), ctypes.c_ulong(w))
    return r


def merge(lib, rles):
    arr = (RLE * len(rles))(*rles)
    m = RLE()
    lib.rleMerge(arr, ctypes.byref(m), ctypes.c_ulong(len(rles)), ctypes.c_int(0))
    return m


def decoded_runs(lib, r, h, w):
    """rleDecode into a zeroed image (as _mask.decode allocates it), then rleEncode -> (runs, rleArea)"""
    assert int(counts_of(r).astype(np.int64).sum()) <= h * w
    img = np.zeros(h * w, dtype=np.uint8)
    lib.rleDecode(ctypes.byref(r), img.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(1))
    e = RLE()
    lib.rleEncode(ctypes.byref(e), img.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(h), ctypes.c_ulong(w), ctypes.c_ulong(1))
    a = ctypes.c_uint(0)
    lib.rleArea(ctypes.byref(e), ctypes.c_ulong(1), ctypes.byref(a))
    return counts_of(e), int(a.value)


STYLES = ('inside', 'outside', 'integer', 'half', 'repeat')


def random_polygon(rng, h, w, k, style):
    if style == 'inside':
        xy = np.stack([rng.uniform(0, w, k), rng.uniform(0, h, k)], 1)
    elif style == 'outside':
        xy = np.stack([rng.uniform(-0.8 * w - 3, 1.8 * w + 3, k), rng.uniform(-0.8 * h - 3, 1.8 * h + 3, k)], 1)
    elif style == 'integer':
        xy = np.stack([rng.randint(-1, w + 2, k), rng.randint(-1, h + 2, k)], 1).astype(np.float64)
    elif style == 'half':
        xy = np.stack([rng.randint(-1, w + 2, k), rng.randint(-1, h + 2, k)], 1) + 0.5
    else:
        xy = np.stack([rng.uniform(-1, w + 1, k), rng.uniform(-1, h + 1, k)], 1).round(1)
        if k > 1:
            xy[rng.randint(k), rng.randint(2)] = xy[rng.randint(k), rng.randint(2)]      # a repeated coordinate
            if k < 8:
                j = rng.randint(k)
                xy = np.insert(xy, j, xy[j], axis=0)                                        # a duplicate vertex
    return xy


def with_duplicate(rng, xy):
    """the polygon with one vertex inserted again: exactly, or closer than the 1/5-pixel grid resolves"""
    j = rng.randint(len(xy))
    extra = xy[j] + (0.0 if rng.rand() < 0.5 else rng.uniform(-0.04, 0.04, 2))
    return np.insert(xy, j + 1, extra, axis=0)


def column_end_boundaries(runs, h, w):
    cc = np.cumsum(runs.astype(np.int64))[:-1]
    return int(((cc % h == 0) & (cc > 0) & (cc < h * w)).sum())


def ellipse(cx, cy, rx, ry, k):
    a = np.arange(k) * (2 * np.pi / k)
    return np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], 1)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SCDA_REFERENCE", "/root/reference")
    rng = np.random.RandomState(2024)
    cases = []                                  # (group, h, w, [polygons], kind, rle counts or None, string or None)
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_reference(ref_root, tmp)

        def poly_runs(xy, h, w):
            return decoded_runs(lib, fr_poly(lib, xy, h, w), h, w)[0]

        # a
        for i in range(200):
            h, w = (1, 1) if i == 0 else (40, 70) if i == 1 else (rng.randint(1, 41), rng.randint(1, 71))
            cases.append(('a', h, w, [random_polygon(rng, h, w, rng.randint(1, 9), STYLES[i % 5])], 0, None, None))
        # b, c, d
        cases.append(('b', 10, 10, [np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float64)], 0, None, None))
        cases.append(('c', 7, 9, [np.array([[-50, -40], [70, -45], [66, 52], [-48, 61]], np.float64)], 0, None, None))
        cases.append(('d', 12, 17, [np.array([[3.2, 4.1]])], 0, None, None))
        cases.append(('d', 12, 17, [np.array([[3.2, 4.1], [9.7, 10.3]])], 0, None, None))
        cases.append(('d', 12, 17, [np.array([[5.0, 1.0], [5.0, 11.0], [5.0, 6.0]])], 0, None, None))
        # e: a seeded search for duplicates that change the reference's mask
        found = tries = 0
        while found < 6:
            tries += 1
            h, w = rng.randint(6, 41), rng.randint(6, 71)
            xy = random_polygon(rng, h, w, rng.randint(3, 8), 'inside')
            dup = with_duplicate(rng, xy)
            if not np.array_equal(poly_runs(xy, h, w), poly_runs(dup, h, w)):
                cases.append(('e', h, w, [dup], 0, None, None))
                cases.append(('e', h, w, [xy], 0, None, None))
                found += 1
        print("e: %d duplicates that change the mask in %d tries" % (found, tries))
        # f: run boundaries on column ends
        for h, w in ((5, 33), (37, 70)):
            cases.append(('f', h, w, [np.array([[2, 0], [w - 3, 0], [w - 3, h], [2, h]], np.float64)], 0, None, None))   # full-height box
            found = 0
            while found < 4:
                style = STYLES[rng.randint(5)]
                xy = random_polygon(rng, h, w, rng.randint(3, 9), style)
                if column_end_boundaries(poly_runs(xy, h, w), h, w) > 0:
                    cases.append(('f', h, w, [xy], 0, None, None))
                    found += 1
        # g: annotations of several polygons
        for n_poly in (2, 3, 4, 2, 3, 4):
            h, w = rng.randint(12, 41), rng.randint(20, 71)
            polys = [random_polygon(rng, h, w, rng.randint(3, 9), 'inside') for _ in range(n_poly)]
            cases.append(('g', h, w, polys, 0, None, None))
        h, w = 30, 64                            # disjoint parts, one of them degenerate
        cases.append(('g', h, w, [np.array([[1, 1], [10, 2], [6, 12]], np.float64), np.array([[40, 15], [60, 15], [60, 28], [40, 28]], np.float64),
                                   np.array([[20.5, 20.5], [20.5, 20.5]])], 0, None, None))
        # h: uncompressed RLEs / i: the same as strings
        rles = [(5, 33, [0, 7, 3, 5, 150]), (5, 33, [160, 5]), (5, 33, [4, 1, 0, 3, 20, 10]), (37, 70, [0, 2590]), (37, 70, [2590]),
                (37, 70, [36, 2, 35, 74, 1000, 443]), (37, 70, [100, 200, 300, 400, 500, 1, 0, 1, 7]), (1, 1, [0, 1]), (40, 70, [2799, 1]),
                (9, 31, list(rng.randint(0, 9, 40)))]
        for h, w, c in rles:
            assert sum(c) <= h * w
            cases.append(('h', h, w, [], 1, np.asarray(c, np.uint32), None))
        big = [3, 1, 40, 2, 700, 5, 20000, 1, 600000, 30, 7, 20000, 1, 400, 9, 15, 300, 16, 1, 1, 17000, 2]
        for h, w, c in rles + [(800, 1344, big), (800, 1344, big + [800 * 1344 - sum(big) - 5, 5])]:
            lib.rleToString.restype = ctypes.c_char_p
            s = lib.rleToString(ctypes.byref(make_rle(c, h, w)))
            cases.append(('i', h, w, [], 2, None, bytes(s)))
        # j
        H, W = 800, 1344
        cases.append(('j', H, W, [ellipse(650.3, 410.7, 560.0, 330.0, 64)], 0, None, None))
        cases.append(('j', H, W, [np.array([[0.0, 0.0], [1344.0, 800.0], [900.5, 790.25], [10.0, 300.0]]),
                                  ellipse(1100.0, 200.0, 300.0, 150.0, 23),
                                  np.array([[100.2, 500.1], [400.9, 480.3], [420.0, 799.9], [250.5, 640.0], [90.0, 780.6]])], 0, None, None))

        out = {k: [] for k in ('xy', 'rle_counts', 'str_bytes', 'out_counts', 'frpoly_counts')}
        firsts = {k: [0] for k in ('poly', 'vert', 'rle', 'str', 'out', 'frpoly')}
        group, size, bigf, kind, area = [], [], [], [], []
        n_pos = {k: 0 for k in out}

        def push(name, key, values):
            out[key].append(values)
            n_pos[key] += len(values)
            firsts[name].append(n_pos[key])

        for g, h, w, polys, kd, counts, s in cases:
            group.append(g); size.append((h, w)); bigf.append(h * w > 40 * 96); kind.append(kd)
            frpoly = np.zeros(0, np.uint32)
            if kd == 0:
                rs = []
                for xy in polys:
                    xy = np.asarray(xy, np.float64).reshape(-1, 2)
                    push('vert', 'xy', xy)
                    rs.append(fr_poly(lib, xy, h, w))
                r = merge(lib, rs)
                if len(polys) == 1:
                    frpoly = counts_of(rs[0])
                counts_in = np.zeros(0, np.uint32)
            elif kd == 1:
                r, counts_in = make_rle(counts, h, w), counts
            else:
                r = RLE()
                lib.rleFrString(ctypes.byref(r), ctypes.c_char_p(s), ctypes.c_ulong(h), ctypes.c_ulong(w))
                counts_in = counts_of(r)
            firsts['poly'].append(firsts['poly'][-1] + len(polys))
            push('rle', 'rle_counts', counts_in)
            push('str', 'str_bytes', np.frombuffer(s or b'', dtype=np.uint8))
            runs, a = decoded_runs(lib, r, h, w)
            if len(polys) == 1:
                assert np.array_equal(frpoly, runs), (g, frpoly, runs)           # rleFrPoly's counts are canonical
            push('out', 'out_counts', runs)
            push('frpoly', 'frpoly_counts', frpoly)
            area.append(a)
    res = {'group': np.asarray(group), 'size': np.asarray(size, np.int32), 'big': np.asarray(bigf, np.uint8), 'kind': np.asarray(kind, np.uint8),
           'area': np.asarray(area, np.uint32), 'xy': np.concatenate(out['xy']).astype(np.float64)}
    for key in ('rle_counts', 'out_counts', 'frpoly_counts'):
        res[key] = np.concatenate(out[key]).astype(np.uint32)
    res['str_bytes'] = np.concatenate(out['str_bytes']).astype(np.uint8)
    for name, v in firsts.items():
        res[name + '_first'] = np.asarray(v, np.int32)
    path = os.path.join(HERE, "mask_poly_ref.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", int(res['big'].sum()), "big;",
          {g: int((res['group'] == g).sum()) for g in sorted(set(group))})


if __name__ == "__main__":
    main()
