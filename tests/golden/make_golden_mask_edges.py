"""Generates tests/golden/mask_edges_ref.npz: the case table of tests/mask_edge_cases.py through the REFERENCE's run-length code.
datasets/pycocotools/common/maskApi.c is compiled UNMODIFIED into a temporary directory exactly as make_golden_mask_rle.py does
(load_reference) and called through ctypes.  Run in the build container:
    python tests/golden/make_golden_mask_edges.py [path of the reference checkout]

Neither the C file nor the library is kept.  The file holds inputs and recorded outputs only:
  enc_*    the encoder cases (section 1a): name, size, the clean packed plane, rleEncode counts, rleToString bytes, rleArea, rleToBbox
  wide_*   four planes of 3 rows x 320 columns (a second round of the 256-column scan), the same outputs
  b300_*   the 300 planes of [3, 1] words with their 100 image_info rows, the same outputs
  hint_*   the hint-window cases (1b): name, size, roi row, plane, the same outputs
  large_*  the 4100 x 4100 plane with six-character differences (1c): its OUTPUTS only, the plane is built from parameters
  iou_<h>x<w>_*  the IoU sets (1d): dt / gt planes, rleIou with iscrowd = (g % 2) and with 1 - that, the raw intersections (rleArea of
           rleMerge(intersect = 1)); iou_m70_* the 70 x 3 set
  poly_* / polybig_*   the annToMask cases (1e) on 66 x 96 planes and the four 363 x 384 planes: name, size, vertices, counts,
           strings; the decoded plane (rleDecode of rleMerge of rleFrPoly / frUncompressedRLE / rleFrString), rleArea, rleFrString's
           counts, and rleFrPoly's own counts for single-polygon planes
An empty polygon slot is not handed to rleFrPoly (the reference never calls it with k = 0); the inputs that the reference does not
define (tests/test_mask_edges_gpu.py builds them) are not here at all."""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_mask_rle import load_reference, pack, ref_iou, ref_outputs   # noqa: E402
from make_golden_mask_poly import RLE, counts_of, fr_poly, make_rle, merge    # noqa: E402
import mask_edge_cases as E                                                   # noqa: E402


def record(out, prefix, results):
    """results: [(counts, chars, area, bbox)] of ref_outputs"""
    out[prefix + '_counts'], out[prefix + '_first'] = E.ragged([r[0] for r in results], np.uint32)
    out[prefix + '_chars'], out[prefix + '_cfirst'] = E.ragged([r[1] for r in results], np.uint8)
    out[prefix + '_area'] = np.asarray([r[2] for r in results], dtype=np.uint32)
    out[prefix + '_bbox'] = np.stack([r[3] for r in results])


def decoded(lib, r, h, w):
    """rleDecode into a zeroed image (as _mask.decode allocates it) -> (bool [h, w], rleArea)"""
    assert int(counts_of(r).astype(np.int64).sum()) <= h * w
    img = np.zeros(h * w, dtype=np.uint8)
    lib.rleDecode(ctypes.byref(r), img.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(1))
    e = RLE()
    lib.rleEncode(ctypes.byref(e), img.ctypes.data_as(ctypes.c_void_p), ctypes.c_ulong(h), ctypes.c_ulong(w), ctypes.c_ulong(1))
    a = ctypes.c_uint(0)
    lib.rleArea(ctypes.byref(e), ctypes.c_ulong(1), ctypes.byref(a))
    return img.reshape(w, h).T.astype(bool), int(a.value)


def ann_to_mask(lib, out, prefix, planes, H, Wd):
    for k, v in E.flat_annotations(planes).items():
        out[prefix + '_' + k] = v
    out[prefix + '_name'] = np.asarray(['' if c is None else c['name'] for c in planes])
    lib.rleToString.restype = ctypes.c_char_p
    bits, area, frpoly, strings, str_counts = [], [], [], [], []
    for c in planes:
        fp, s, sc = np.zeros(0, np.uint32), b'', np.zeros(0, np.uint32)
        if c is None:
            bits.append(np.zeros((H, Wd), np.uint32)); area.append(0)
        else:
            h, w = c['h'], c['w']
            rs = [fr_poly(lib, p, h, w) for p in c['polygons'] if len(p)]
            if len(c['polygons']) == 1:
                fp = counts_of(rs[0])
            if c['string'] is not None:
                s = bytes(lib.rleToString(ctypes.byref(make_rle(c['counts'], h, w))))
                assert s == c['string'], (c['name'], s, c['string'])          # the table's string is the reference's
                r = RLE()
                lib.rleFrString(ctypes.byref(r), ctypes.c_char_p(s), ctypes.c_ulong(h), ctypes.c_ulong(w))
                sc = counts_of(r)
                rs.append(r)
            elif c['counts'] is not None:
                rs.append(make_rle(c['counts'], h, w))
            m, a = decoded(lib, merge(lib, rs) if len(rs) > 1 else rs[0], h, w)
            bits.append(pack(m, H, Wd)); area.append(a)
        frpoly.append(fp); strings.append(np.frombuffer(s, dtype=np.uint8)); str_counts.append(sc)
    out[prefix + '_bits'] = np.stack(bits)
    out[prefix + '_area'] = np.asarray(area, dtype=np.uint32)
    out[prefix + '_frpoly'], out[prefix + '_frpoly_first'] = E.ragged(frpoly, np.uint32)
    out[prefix + '_str'], out[prefix + '_str_first'] = E.ragged(strings, np.uint8)
    out[prefix + '_str_counts'], out[prefix + '_str_counts_first'] = E.ragged(str_counts, np.uint32)


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SCDA_REFERENCE", "/root/reference")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_reference(ref_root, tmp)
        # 1a
        enc = E.encoder_cases()
        out['enc_name'] = np.asarray([c['name'] for c in enc])
        out['enc_size'] = np.asarray([(c['h'], c['w']) for c in enc], dtype=np.int32)
        out['enc_bits'] = np.stack([pack(c['mask'], E.H, E.WD) for c in enc])
        record(out, 'enc', [ref_outputs(lib, c['mask']) for c in enc])
        bits, info = E.batch300()
        out['b300_bits'], out['b300_info'] = bits, info
        record(out, 'b300', [ref_outputs(lib, E.R.unpack(bits[r], int(info[r // 3, 0]), int(info[r // 3, 1]))) for r in range(300)])
        bits, info = E.wide_batch()
        out['wide_bits'], out['wide_info'] = bits, info
        record(out, 'wide', [ref_outputs(lib, E.R.unpack(bits[r], int(info[r, 0]), int(info[r, 1]))) for r in range(len(bits))])
        # 1b
        hint = E.hint_cases()
        out['hint_name'] = np.asarray([c['name'] for c in hint])
        out['hint_size'] = np.asarray([(c['h'], c['w']) for c in hint], dtype=np.int32)
        out['hint_roi'] = np.stack([c['roi'] for c in hint])
        out['hint_bits'] = np.stack([pack(c['mask'], E.H, E.WD) for c in hint])
        record(out, 'hint', [ref_outputs(lib, c['mask']) for c in hint])
        # 1c
        record(out, 'large', [ref_outputs(lib, E.large_mask())])
        # 1d
        for i, (h, w) in enumerate(E.IOU_SIZES):
            names, dt, gt = E.iou_masks(h, w, 900 + i)
            key = 'iou_%dx%d' % (h, w)
            out[key + '_name'] = np.asarray(names)
            out[key + '_dt'] = np.stack([pack(m, E.H, E.WD) for m in dt])
            out[key + '_gt'] = np.stack([pack(m, E.H, E.WD) for m in gt])
            crowd = E.iou_crowd(len(gt))
            out[key + '_o0'], out[key + '_inter'] = ref_iou(lib, list(dt), list(gt), crowd)
            out[key + '_o1'], again = ref_iou(lib, list(dt), list(gt), 1 - crowd)
            assert np.array_equal(again, out[key + '_inter'])
        dt, gt, crowd = E.iou_m70()
        out['iou_m70_dt'] = np.stack([pack(m, E.H, E.WD) for m in dt])
        out['iou_m70_gt'] = np.stack([pack(m, E.H, E.WD) for m in gt])
        out['iou_m70_iscrowd'] = crowd
        out['iou_m70_o'], out['iou_m70_inter'] = ref_iou(lib, list(dt), list(gt), crowd)
        # 1e
        ann_to_mask(lib, out, 'poly', E.poly_cases(), E.H, E.WD)
        ann_to_mask(lib, out, 'polybig', E.poly_big_cases(), E.BIG['H'], E.BIG['Wd'])
    path = os.path.join(HERE, "mask_edges_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(enc), "encoder,", len(hint), "hint,", len(out['poly_name']), "annToMask planes")
    print("large:", out['large_counts'].tolist(), out['large_chars'].tobytes(), out['large_bbox'].tolist())


if __name__ == "__main__":
    main()
