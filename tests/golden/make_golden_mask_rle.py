"""Generates tests/golden/mask_rle_ref.npz with the REFERENCE's run-length code: datasets/pycocotools/common/maskApi.c is compiled
UNMODIFIED with the system C compiler into a temporary directory (gcc -O2 -fPIC -shared -std=c99 -I<common>) and rleEncode,
rleToString, rleArea, rleToBbox, rleMerge (for the raw intersections) and rleIou are called through ctypes.  Run in the build container:
    python tests/golden/make_golden_mask_rle.py [path of the reference checkout]

Neither the C file nor the library is kept.  The file holds inputs (masks bit-packed as scda_mask_paste_hip packs them, with the image
size of every mask) and the recorded outputs only.  Groups of planes [n, H, Wd]:
  small  12 x 32 planes: empty, full, the four corners, one row, one column, the wrapped-run mask (10 x 6, [5:, 1] and [:4, 2]) and the
         mask that its box gate zeroes ([7:9, 1]), random planes with crops h_r < H, w_r < 32 Wd and set bits outside the crop
  mid    70 x 96 planes, sizes that are no multiples of 32 / 64: densities 0.02 / 0.5 / 0.98, a checkerboard, stripes
  big    800 x 1344: ellipses, a threshold of smooth noise (blobs), boxes, a crop, and a mask built from runs whose counts and
         differences need 1, 2, 3, 4 and 5 characters, negative differences included
IoU sets (dt, gt, size, iscrowd or none): the wrapped pair, a mid set with identical and disjoint pairs, a big set."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class RLE(ctypes.Structure):
    _fields_ = [("h", ctypes.c_ulong), ("w", ctypes.c_ulong), ("m", ctypes.c_ulong), ("cnts", ctypes.POINTER(ctypes.c_uint))]


def load_reference(ref_root, tmp):
    common = os.path.join(ref_root, "datasets", "pycocotools", "common")
    so = os.path.join(tmp, "libmaskapi.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c99", "-I" + common, os.path.join(common, "maskApi.c"), "-o", so, "-lm"])
    lib = ctypes.CDLL(so)
    lib.rleToString.restype = ctypes.c_char_p          # (the string's storage is the C library's; the process is short-lived)
    return lib


def pack(mask, H, Wd):
    """bool [h, w] -> uint32 [H, Wd]"""
    full = np.zeros((H, Wd * 32), dtype=np.uint8)
    full[:mask.shape[0], :mask.shape[1]] = mask
    return np.packbits(full, axis=-1, bitorder='little').view(np.uint32).reshape(H, Wd)


def ref_rle(lib, mask):
    h, w = mask.shape
    m = np.asfortranarray(mask.astype(np.uint8))
    r = RLE()
    lib.rleEncode(ctypes.byref(r), m.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(h), ctypes.c_ulong(w), ctypes.c_ulong(1))
    return r


def ref_outputs(lib, mask):
    r = ref_rle(lib, mask)
    counts = np.array([r.cnts[i] for i in range(r.m)], dtype=np.uint32)
    chars = np.frombuffer(lib.rleToString(ctypes.byref(r)), dtype=np.uint8).copy()
    a = ctypes.c_uint(0)
    lib.rleArea(ctypes.byref(r), ctypes.c_ulong(1), ctypes.byref(a))
    bb = (ctypes.c_double * 4)()
    lib.rleToBbox(ctypes.byref(r), bb, ctypes.c_ulong(1))
    return counts, chars, int(a.value), np.array(list(bb), dtype=np.float64)


def ref_iou(lib, dts, gts, iscrowd):
    M, N = len(dts), len(gts)
    D = (RLE * M)(*[ref_rle(lib, m) for m in dts])
    G = (RLE * N)(*[ref_rle(lib, m) for m in gts])
    o = np.zeros(N * M, dtype=np.float64)
    crowd = None if iscrowd is None else np.ascontiguousarray(iscrowd, dtype=np.uint8)
    lib.rleIou(D, G, ctypes.c_ulong(M), ctypes.c_ulong(N), None if crowd is None else crowd.ctypes.data_as(ctypes.c_void_p),
               o.ctypes.data_as(ctypes.c_void_p))
    inter = np.zeros((N, M), dtype=np.uint32)
    for g in range(N):
        for d in range(M):
            pair = (RLE * 2)(D[d], G[g])
            merged = RLE()
            lib.rleMerge(pair, ctypes.byref(merged), ctypes.c_ulong(2), ctypes.c_int(1))
            a = ctypes.c_uint(0)
            lib.rleArea(ctypes.byref(merged), ctypes.c_ulong(1), ctypes.byref(a))
            inter[g, d] = a.value
    return o.reshape(N, M), inter


def from_runs(runs, h, w):
    """bool [h, w] whose column-major runs are `runs` (zeros first), the rest zeros"""
    flat = np.zeros(h * w, dtype=bool)
    p, v = 0, False
    for n in runs:
        flat[p:p + n] = v
        p += n
        v = not v
    assert p <= h * w
    return flat.reshape(w, h).T.copy()


def small_cases(rng):
    h, w = 10, 6
    z = lambda: np.zeros((h, w), dtype=bool)                                  # noqa: E731
    cases = [z(), ~z()]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = z(); m[y, x] = True; cases.append(m)
    m = z(); m[4, :] = True; cases.append(m)
    m = z(); m[:, 3] = True; cases.append(m)
    m = z(); m[5:, 1] = True; m[:4, 2] = True; cases.append(m)                # the run wraps from column 1 into column 2
    m = z(); m[7:9, 1] = True; cases.append(m)
    m = z(); m[:, 0] = True; m[:, w - 1] = True; cases.append(m)
    sizes = [(h, w)] * len(cases)
    planes = [pack(c, 12, 1) for c in cases]
    for hh, ww, dens in ((7, 5, 0.5), (12, 32, 0.5), (11, 31, 0.9), (1, 32, 0.5), (12, 1, 0.5), (1, 1, 1.0), (3, 17, 0.1)):
        full = rng.rand(12, 32) < dens                                        # bits outside the crop stay set in the plane
        cases.append(full[:hh, :ww].copy()); sizes.append((hh, ww)); planes.append(pack(full, 12, 1))
    return cases, sizes, planes


def mid_cases(rng):
    H, Wd = 70, 3
    cases, sizes, planes = [], [], []
    for (hh, ww) in ((70, 96), (67, 83), (33, 65), (64, 64)):
        for dens in (0.02, 0.5, 0.98):
            full = rng.rand(H, Wd * 32) < dens
            cases.append(full[:hh, :ww].copy()); sizes.append((hh, ww)); planes.append(pack(full, H, Wd))
        yy, xx = np.mgrid[:H, :Wd * 32]
        for full in ((yy + xx) % 2 == 0, (yy + xx) % 2 == 1, yy % 2 == 0, xx % 3 == 0):
            cases.append(full[:hh, :ww].copy()); sizes.append((hh, ww)); planes.append(pack(full, H, Wd))
    return cases, sizes, planes


def big_cases(rng):
    H, W = 800, 1344
    yy, xx = np.mgrid[:H, :W]
    cases = [((yy - 400.0) / 380.0) ** 2 + ((xx - 672.0) / 499.5) ** 2 <= 1.0,          # 999 columns wide
             ((yy - 90.0) / 60.0) ** 2 + ((xx - 1300.0) / 80.0) ** 2 <= 1.0]            # cut by the right border
    # smooth noise: a coarse random field enlarged by linear interpolation, thresholded -> blobs
    coarse = rng.rand(11, 17)
    gy, gx = np.linspace(0, 10, H), np.linspace(0, 16, W)
    y0, x0 = np.minimum(gy.astype(int), 9), np.minimum(gx.astype(int), 15)
    fy, fx = (gy - y0)[:, None], (gx - x0)[None, :]
    field = (coarse[y0][:, x0] * (1 - fy) * (1 - fx) + coarse[y0 + 1][:, x0] * fy * (1 - fx)
             + coarse[y0][:, x0 + 1] * (1 - fy) * fx + coarse[y0 + 1][:, x0 + 1] * fy * fx)
    cases.append(field > 0.6)
    m = np.zeros((H, W), dtype=bool); m[100:300, 200:900] = True; cases.append(m)
    m = np.zeros((H, W), dtype=bool); m[0:800, 1300:1344] = True; m[0:17, 0:3] = True; cases.append(m)   # touches the last pixel
    # counts / differences of 1 .. 5 characters, both signs: |x| < 16, < 512, < 16384, < 524288, above
    cases.append(from_runs([3, 1, 40, 2, 700, 5, 20000, 1, 600000, 30, 7, 20000, 1, 400, 9, 15, 300, 16, 1, 1, 17000, 2], H, W))
    sizes = [(H, W)] * len(cases)
    planes = [pack(c, H, W // 32) for c in cases]
    full = cases[2] | cases[3]                                                # a crop with set bits outside
    cases.append(full[:750, :1333].copy()); sizes.append((750, 1333)); planes.append(pack(full, H, W // 32))
    return cases, sizes, planes


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SCDA_REFERENCE", "/root/reference")
    rng = np.random.RandomState(77)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_reference(ref_root, tmp)
        groups = {'small': small_cases(rng), 'mid': mid_cases(rng), 'big': big_cases(rng)}
        for name, (cases, sizes, planes) in groups.items():
            res = [ref_outputs(lib, c) for c in cases]
            out[name + '_bits'] = np.stack(planes)
            out[name + '_sizes'] = np.asarray(sizes, dtype=np.int32)
            out[name + '_n_runs'] = np.asarray([len(r[0]) for r in res], dtype=np.int32)
            out[name + '_counts'] = np.concatenate([r[0] for r in res])
            out[name + '_n_bytes'] = np.asarray([len(r[1]) for r in res], dtype=np.int32)
            out[name + '_chars'] = np.concatenate([r[1] for r in res])
            out[name + '_area'] = np.asarray([r[2] for r in res], dtype=np.uint32)
            out[name + '_bbox'] = np.stack([r[3] for r in res])
        # IoU sets: indices into a group's masks of ONE size
        small, mid, big = groups['small'][0], groups['mid'][0], groups['big'][0]
        sets = {'wrap': ('small', [8, 1, 6], [9, 8, 0, 7], None),
                'wrap_crowd': ('small', [8, 1, 6], [9, 8, 0, 7], [1, 0, 1, 0]),
                'mid': ('mid', [0, 1, 2, 3, 4], [1, 2, 3, 4, 5, 6], None),
                'mid_crowd': ('mid', [0, 1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [0, 1, 0, 1, 1, 0]),
                'big': ('big', [0, 1, 2, 3], [0, 3, 4, 5, 1], None),
                'big_crowd': ('big', [0, 1, 2, 3], [0, 3, 4, 5, 1], [1, 0, 0, 1, 1])}
        for name, (grp, di, gi, crowd) in sets.items():
            cases, sizes, _ = groups[grp]
            assert len({sizes[i] for i in di + gi}) == 1
            o, inter = ref_iou(lib, [cases[i] for i in di], [cases[i] for i in gi], crowd)
            out['iou_%s_group' % name] = np.asarray(grp)
            out['iou_%s_dt' % name] = np.asarray(di, dtype=np.int32)
            out['iou_%s_gt' % name] = np.asarray(gi, dtype=np.int32)
            out['iou_%s_iscrowd' % name] = np.asarray([] if crowd is None else crowd, dtype=np.uint8)
            out['iou_%s_o' % name] = o
            out['iou_%s_inter' % name] = inter
    path = os.path.join(HERE, "mask_rle_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: int(out[k + '_n_runs'].max()) for k in groups}, "max runs")
    print("wrapped mask bbox", out['small_bbox'][8], " gated pair iou", out['iou_wrap_o'][0, 0], "inter", out['iou_wrap_inter'][0, 0])


if __name__ == "__main__":
    main()
