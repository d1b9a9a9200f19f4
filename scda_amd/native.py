"""ctypes binding of libscda_ops.so (C ABI declared in include/scda_ops.h).

lib() reads that header when it loads the library and sets `argtypes` / `restype` of every declared function from its declaration:
the signatures are stated once, in the header, and a call site passes plain Python values (ctypes converts them to the declared C
types and raises on a missing argument or a value of the wrong kind).

Every wrapper takes torch CUDA tensors, checks device/dtype/contiguity, passes
raw device pointers + sizes + the current HIP stream, and raises on a non-zero
status.  There is no CPU fallback: operators raise if the library or a HIP
device is missing.
"""
import ctypes
import os
import re
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCDA_OPS_LIB") or os.path.join(_HERE, "libscda_ops.so")   # (the env override: A/B builds of the library)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "scda_ops.h")            # always this checkout's

_lib = None


class ScdaNativeError(RuntimeError):
    pass


# the header's whole type vocabulary; every pointer or array parameter is a c_void_p (an int address, None, a ctypes array or byref())
C_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
             "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}
C_RETURNS = dict(C_SCALARS, **{"void": None, "const char *": ctypes.c_char_p})


def parse_header(text):
    """{function name: (restype, [argtypes])} of the declarations in the text of a plain-C header"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'^\s*#.*$|extern\s*"C"\s*\{|\}', " ", text, flags=re.M)
    sigs = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\(([^()]*)\)", decl)
        if not m or m.group(1).strip() not in C_RETURNS:
            raise ScdaNativeError(f"cannot bind the declaration `{decl}`: not `<{' | '.join(C_RETURNS)}> name(parameters)`")
        argtypes = []
        for param in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            ctype = " ".join(w for w in param.split()[:-1] if w != "const")      # the last word is the parameter's name
            if "*" in param or param.rstrip().endswith("]"):
                argtypes.append(ctypes.c_void_p)
            elif ctype in C_SCALARS:
                argtypes.append(C_SCALARS[ctype])
            else:
                raise ScdaNativeError(f"cannot bind the declaration `{decl}`: parameter `{param.strip()}` has no type in {sorted(C_SCALARS)}")
        sigs[m.group(2)] = (C_RETURNS[m.group(1).strip()], argtypes)
    return sigs


def lib():
    """Load libscda_ops.so once and type every function include/scda_ops.h declares; fail loudly if either is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ScdaNativeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C scda_amd/csrc` (no CPU fallback exists)")
        if not os.path.exists(HEADER_PATH):
            raise ScdaNativeError(f"{HEADER_PATH} not found: the binding takes every signature of {LIB_PATH} from it")
        cdll = ctypes.CDLL(LIB_PATH)
        with open(HEADER_PATH) as f:
            sigs = parse_header(f.read())
        for name, (restype, argtypes) in sigs.items():
            fn = getattr(cdll, name, None)      # a symbol the library lacks raises AttributeError where it is used (tests/test_abi.py lists them)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = cdll
    return _lib


def _check(status, what):
    if status != 0:
        msg = lib().scda_last_error().decode("utf-8", "replace")
        raise ScdaNativeError(f"{what} failed with status {status}: {msg}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """current HIP stream of the current device as an address (one C call; this runs once per kernel launch)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t is not None else None


def _req(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise ScdaNativeError(f"{name} must live on the HIP device (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


# ----------------------------------------------------------------- NMS ------
def nms(boxes, thresh, max_keep=0):
    """boxes [n,5] fp32 CUDA, sorted by score desc -> (keep int64[n] CUDA, num_out int64[1] CUDA)."""
    _req(boxes, "boxes")
    n = boxes.shape[0]
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=boxes.device)
    num = torch.zeros(1, dtype=torch.int64, device=boxes.device)
    ws = torch.empty(max(lib().scda_nms_workspace_bytes(n), 8), dtype=torch.uint8, device=boxes.device)
    _check(lib().scda_nms_hip(_p(boxes), n, thresh, _p(ws), _p(keep), _p(num), max_keep, _stream()), "scda_nms_hip")
    return keep, num


def nms_segments(boxes, seg, max_n, thresh):
    """S independent score-sorted lists in one mask + one sweep launch (scda_nms_segments_hip): boxes [rows,5] fp32 CUDA (the lists
    back to back), seg int64 [S,3] CUDA = (first row, length, first mask word) -> (keep int64 [rows] CUDA, num int64 [S] CUDA)"""
    _req(boxes, "boxes"); _req(seg, "seg", torch.int64)
    S, rows = seg.shape[0], boxes.shape[0]
    keep = torch.empty(max(rows, 1), dtype=torch.int64, device=boxes.device)
    num = torch.zeros(max(S, 1), dtype=torch.int64, device=boxes.device)
    words = S * max_n * ((max_n + 63) // 64)                  # upper bound of the lists' mask words
    ws = torch.empty(max(words, 1), dtype=torch.int64, device=boxes.device)
    _check(lib().scda_nms_segments_hip(_p(boxes), _p(seg), S, max_n, thresh, _p(ws), _p(keep), _p(num), _stream()), "scda_nms_segments_hip")
    return keep, num


SOFT_NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}
SOFT_NMS_DEFAULTS = {"method": "hard", "sigma": 0.5, "Nt": 0.3, "threshold": 0.001}       # the reference's (cython_nms.pyx:98-104)


def soft_nms_capacity():
    """rows of one list the soft-NMS kernel holds in LDS"""
    return int(lib().scda_soft_nms_capacity())


def soft_nms_setting(spec):
    """a `soft_nms` setting -> None (hard NMS as ever) or (method 0..2, sigma, Nt, threshold).  spec: None, or a dict with any of
    'method' ('hard' | 'linear' | 'gaussian' or 0 | 1 | 2), 'sigma', 'Nt', 'threshold'; what it leaves out takes the reference's
    default (method 0 -- the sweep's own hard rule, ov > Nt drops --, sigma 0.5, Nt 0.3, threshold 0.001).  ValueError for an unknown
    key or method and a sigma <= 0."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError("soft_nms: expected None or a dict of %s, got %r" % (sorted(SOFT_NMS_DEFAULTS), spec))
    unknown = sorted(set(spec) - set(SOFT_NMS_DEFAULTS))
    if unknown:
        raise ValueError("soft_nms: unknown keys %s (known: %s)" % (unknown, sorted(SOFT_NMS_DEFAULTS)))
    s = dict(SOFT_NMS_DEFAULTS, **spec)
    m = s["method"]
    if isinstance(m, str):
        if m not in SOFT_NMS_METHODS:
            raise ValueError("soft_nms: unknown method %r (one of %s)" % (m, sorted(SOFT_NMS_METHODS)))
        m = SOFT_NMS_METHODS[m]
    if isinstance(m, bool) or m not in (0, 1, 2):
        raise ValueError("soft_nms: unknown method %r (0 hard, 1 linear, 2 gaussian)" % (s["method"],))
    sigma = float(s["sigma"])
    if not sigma > 0:
        raise ValueError("soft_nms: sigma must be > 0, got %r" % (s["sigma"],))
    return int(m), sigma, float(s["Nt"]), float(s["threshold"])


def soft_nms_segments(boxes, seg, max_n, method, sigma, Nt, threshold):
    """soft-NMS (cython_nms.soft_nms) of S independent lists in one launch (scda_soft_nms_segments_hip): boxes [rows,5] fp32 CUDA (the
    lists back to back, in any order), seg int64 [S,3] CUDA = (first row, length, unused) -> (keep int64 [rows] CUDA: each list's
    surviving rows as local indices in selection order from its first row on, num int64 [S] CUDA); the score column of `boxes` is
    rewritten in place with the survivors' final scores.  method 0 hard, 1 linear, 2 gaussian; max_n <= soft_nms_capacity()."""
    _req(boxes, "boxes"); _req(seg, "seg", torch.int64)
    S, rows = seg.shape[0], boxes.shape[0]
    keep = torch.empty(max(rows, 1), dtype=torch.int64, device=boxes.device)
    num = torch.zeros(max(S, 1), dtype=torch.int64, device=boxes.device)
    _check(lib().scda_soft_nms_segments_hip(_p(boxes), _p(seg), S, max_n, method, sigma, Nt, threshold, _p(keep), _p(num), _stream()),
           "scda_soft_nms_segments_hip")
    return keep, num


def nms_mask(boxes, thresh):
    _req(boxes, "boxes")
    n = boxes.shape[0]
    cb = (n + 63) // 64
    mask = torch.zeros(n, cb, dtype=torch.int64, device=boxes.device)
    _check(lib().scda_nms_mask_hip(_p(boxes), n, thresh, _p(mask), _stream()), "scda_nms_mask_hip")
    return mask


# ------------------------------------------------------------- RoIPool ------
def roi_pool_fwd(features, rois, ph, pw, scale, want_argmax=True):
    """-> (out [R,C,ph,pw], argmax int32 [R,C,ph,pw] | None).  want_argmax=False (nothing will be differentiated through the
    call, e.g. the target-domain branch) skips the second 51 MB output."""
    _req(features, "features"); _req(rois, "rois")
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError("rois must be [R,5]")
    B, C, H, W = features.shape
    R = rois.shape[0]
    out = torch.empty(R, C, ph, pw, dtype=torch.float32, device=features.device)
    arg = torch.empty(R, C, ph, pw, dtype=torch.int32, device=features.device) if want_argmax else None
    _check(lib().scda_roi_pool_fwd_hip(_p(features), _p(rois), R, B, C, H, W, ph, pw, scale, _p(out), _p(arg), _stream()),
           "scda_roi_pool_fwd_hip")
    return out, arg


def roi_pool_bwd(top_grad, argmax, rois, feat_shape, ph, pw, scale):
    _req(top_grad, "top_grad"); _req(argmax, "argmax", torch.int32); _req(rois, "rois")
    B, C, H, W = feat_shape
    R = rois.shape[0]
    gi = torch.empty(B, C, H, W, dtype=torch.float32, device=top_grad.device)
    _check(lib().scda_roi_pool_bwd_hip(_p(top_grad), _p(argmax), _p(rois), R, B, C, H, W, ph, pw, scale, _p(gi), _stream()),
           "scda_roi_pool_bwd_hip")
    return gi


# ------------------------------------------------------------ RoIAlign ------
def roi_align_fwd(features, rois, ah, aw, scale, channel_major=False):
    """-> [R,C,ah,aw], or [C,R,ah,aw] with channel_major (the RoI-head layout of scda_amd/dropin/models/mask_rcnn/resnet.py)"""
    _req(features, "features"); _req(rois, "rois")
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError("rois must be [R,5]")
    B, C, H, W = features.shape
    R = rois.shape[0]
    out = torch.empty((C, R, ah, aw) if channel_major else (R, C, ah, aw), dtype=torch.float32, device=features.device)
    fn = lib().scda_roi_align_cmajor_fwd_hip if channel_major else lib().scda_roi_align_fwd_hip
    _check(fn(_p(features), _p(rois), R, B, C, H, W, ah, aw, scale, _p(out), _stream()), "scda_roi_align_fwd_hip")
    return out


def roi_align_bwd(top_grad, rois, feat_shape, ah, aw, scale, channel_major=False):
    _req(top_grad, "top_grad"); _req(rois, "rois")
    B, C, H, W = feat_shape
    gi = torch.zeros(B, C, H, W, dtype=torch.float32, device=top_grad.device)
    fn = lib().scda_roi_align_cmajor_bwd_hip if channel_major else lib().scda_roi_align_bwd_hip
    _check(fn(_p(top_grad), _p(rois), rois.shape[0], B, C, H, W, ah, aw, scale, _p(gi), _stream()), "scda_roi_align_bwd_hip")
    return gi


# ---------------------------------------------------------- focal loss ------
def focal_sigmoid_fwd(logits, targets, weight_pos, gamma, alpha, num_classes):
    _req(logits, "logits"); _req(targets, "targets", torch.int32)
    losses = torch.empty_like(logits)
    _check(lib().scda_focal_sigmoid_fwd_hip(logits.numel(), _p(logits), _p(targets), weight_pos, gamma, alpha, num_classes, _p(losses),
                                            _stream()), "scda_focal_sigmoid_fwd_hip")
    return losses


def focal_sigmoid_bwd(logits, targets, weight_pos, gamma, alpha, num_classes):
    _req(logits, "logits"); _req(targets, "targets", torch.int32)
    dx = torch.empty_like(logits)
    _check(lib().scda_focal_sigmoid_bwd_hip(logits.numel(), _p(logits), _p(targets), _p(dx), weight_pos, gamma, alpha, num_classes,
                                            _stream()), "scda_focal_sigmoid_bwd_hip")
    return dx


def focal_softmax_fwd(logits, targets, weight_pos, gamma, alpha, num_classes):
    _req(logits, "logits"); _req(targets, "targets", torch.int32)
    rows = logits.numel() // num_classes
    losses = torch.empty(rows, dtype=torch.float32, device=logits.device)
    priors = torch.empty_like(logits)
    _check(lib().scda_focal_softmax_fwd_hip(logits.numel(), _p(logits), _p(targets), weight_pos, gamma, alpha, num_classes, _p(losses),
                                            _p(priors), _stream()), "scda_focal_softmax_fwd_hip")
    return losses, priors


def focal_softmax_bwd(logits, targets, priors, weight_pos, gamma, alpha, num_classes):
    _req(logits, "logits"); _req(targets, "targets", torch.int32); _req(priors, "priors")
    rows = logits.numel() // num_classes
    dx = torch.empty_like(logits)
    buff = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _check(lib().scda_focal_softmax_bwd_hip(logits.numel(), _p(logits), _p(targets), _p(dx), weight_pos, gamma, alpha, num_classes,
                                            _p(priors), _p(buff), _stream()), "scda_focal_softmax_bwd_hip")
    return dx


# -------------------------------------------------------- box overlaps ------
def iou_overlaps(b1, b2):
    _req(b1, "b1"); _req(b2, "b2")
    if b1.shape[1] != b2.shape[1]:
        raise ValueError("box widths differ")
    out = torch.empty(b1.shape[0], b2.shape[0], dtype=torch.float32, device=b1.device)
    _check(lib().scda_iou_overlaps_hip(_p(b1), _p(b2), b1.shape[1], b1.shape[0], b2.shape[0], _p(out), _stream()), "scda_iou_overlaps_hip")
    return out


def bbox_overlaps(boxes, query):
    _req(boxes, "boxes"); _req(query, "query")
    if boxes.shape[1] != 4 or query.shape[1] != 4:
        raise ValueError("bbox_overlaps takes [N,4] and [K,4]")
    out = torch.empty(boxes.shape[0], query.shape[0], dtype=torch.float32, device=boxes.device)
    _check(lib().scda_bbox_overlaps_hip(_p(boxes), boxes.shape[0], _p(query), query.shape[0], _p(out), _stream()), "scda_bbox_overlaps_hip")
    return out


# ------------------------------------------------ box logic on the device ----
def anchor_label(anchors32, gts, neg_thresh, pos_thresh, min_gt_best, bufs):
    """bufs: dict of caller-owned device buffers (best_iou, best_gt, gt_best, labels, pos_list, neg_list, counts)"""
    _req(anchors32, "anchors"); _req(gts, "gts")
    KA, G = anchors32.shape[0], gts.shape[0]
    _check(lib().scda_anchor_label_hip(_p(anchors32), KA, _p(gts), G, gts.shape[1], neg_thresh, pos_thresh, min_gt_best,
                                       _p(bufs["best_iou"]), _p(bufs["best_gt"]), _p(bufs["gt_best"]), _p(bufs["labels"]),
                                       _p(bufs["pos_list"]), _p(bufs["neg_list"]), _p(bufs["counts"]), _stream()), "scda_anchor_label_hip")


def anchor_label_ign(anchors32, gts, neg_thresh, pos_thresh, min_gt_best, anchors64, ign, ign_thresh, bufs):
    """anchor_label with ignore regions (include/scda_ops.h: scda_anchor_label_ign_hip): ign [I, >=4] fp32 rows on the device,
    anchors64 the float64 grid the IoF is taken on, ign_thresh the strict threshold (a double).  ign None: I = 0, which is
    anchor_label"""
    _req(anchors32, "anchors"); _req(gts, "gts")
    I = 0
    if ign is not None:
        _req(ign, "ign"); _req(anchors64, "anchors64", torch.float64)
        I = ign.shape[0]
        if ign.dim() != 2 or ign.shape[1] < 4 or anchors64.shape != anchors32.shape:
            raise ValueError("anchor_label_ign: ign must be [I, >=4] and anchors64 the grid of anchors32")
    KA, G = anchors32.shape[0], gts.shape[0]
    _check(lib().scda_anchor_label_ign_hip(_p(anchors32), KA, _p(gts), G, gts.shape[1], neg_thresh, pos_thresh, min_gt_best,
                                           _p(anchors64) if I else None, _p(ign) if I else None, I, ign.shape[1] if I else 0, ign_thresh,
                                           _p(bufs["best_iou"]), _p(bufs["best_gt"]), _p(bufs["gt_best"]), _p(bufs["labels"]),
                                           _p(bufs["pos_list"]), _p(bufs["neg_list"]), _p(bufs["counts"]), _stream()),
           "scda_anchor_label_ign_hip")


def anchor_finalize(bufs, drop_pos, drop_neg, anchors64, gts, A, fh, fw):
    """-> cls_targets int64 [1,A,fh,fw], loc_targets, loc_masks fp32 [1,4A,fh,fw]"""
    dev = gts.device
    cls_t = torch.empty(1, A, fh, fw, dtype=torch.int64, device=dev)
    loc_t = torch.empty(1, 4 * A, fh, fw, dtype=torch.float32, device=dev)
    loc_m = torch.empty(1, 4 * A, fh, fw, dtype=torch.float32, device=dev)
    _check(lib().scda_anchor_finalize_hip(_p(bufs["labels"]), _p(bufs["best_gt"]), _p(bufs["pos_list"]), _p(drop_pos),
                                          0 if drop_pos is None else drop_pos.numel(), _p(bufs["neg_list"]), _p(drop_neg),
                                          0 if drop_neg is None else drop_neg.numel(), _p(anchors64), _p(gts), gts.shape[1], A, fh, fw,
                                          _p(cls_t), _p(loc_t), _p(loc_m), _stream()), "scda_anchor_finalize_hip")
    return cls_t, loc_t, loc_m


def proposal_match(props, gts, img_h, img_w, pos_thresh, neg_hi, neg_lo, bufs):
    """props [n,>=5] fp32 rows (b,x1,y1,x2,y2,..), gts [G,>=5]; bufs: caller-owned device buffers rois [n+G,4], best_iou, best_gt,
    labels, pos_list, neg_list [n+G], counts [2] (scda_proposal_match_hip)"""
    _req(props, "props"); _req(gts, "gts")
    _check(lib().scda_proposal_match_hip(_p(props), props.shape[0], props.shape[1], _p(gts), gts.shape[0], gts.shape[1], img_h, img_w,
                                         pos_thresh, neg_hi, neg_lo, _p(bufs["rois"]), _p(bufs["best_iou"]), _p(bufs["best_gt"]),
                                         _p(bufs["labels"]), _p(bufs["pos_list"]), _p(bufs["neg_list"]), _p(bufs["counts"]), _stream()),
           "scda_proposal_match_hip")


def proposal_match_ign(props, gts, img_h, img_w, pos_thresh, neg_hi, neg_lo, ign, ign_thresh, bufs):
    """proposal_match with ignore regions (include/scda_ops.h: scda_proposal_match_ign_hip): ign [I, >=4] fp32 rows on the device,
    already filtered by the host; bufs additionally holds ign_flags i8 [n+G], ign_list i32 [n+G], ign_count i32 [2].  ign None:
    I = 0, which is proposal_match (the three extra buffers are not needed then)"""
    _req(props, "props"); _req(gts, "gts")
    I = 0
    if ign is not None:
        _req(ign, "ign")
        I = ign.shape[0]
        if ign.dim() != 2 or ign.shape[1] < 4:
            raise ValueError("proposal_match_ign: ign must be [I, >=4]")
    _check(lib().scda_proposal_match_ign_hip(_p(props), props.shape[0], props.shape[1], _p(gts), gts.shape[0], gts.shape[1], img_h, img_w,
                                             pos_thresh, neg_hi, neg_lo, _p(ign) if I else None, I, ign.shape[1] if I else 0, ign_thresh,
                                             _p(bufs["rois"]), _p(bufs["best_iou"]), _p(bufs["best_gt"]), _p(bufs["labels"]),
                                             _p(bufs["pos_list"]), _p(bufs["neg_list"]), _p(bufs["counts"]),
                                             _p(bufs["ign_flags"]) if I else None, _p(bufs["ign_list"]) if I else None,
                                             _p(bufs["ign_count"]) if I else None, _stream()), "scda_proposal_match_ign_hip")


def proposal_finalize(cand_rois, sel, gt_of, enc, gts, num_classes, image_index):
    """-> rois [R,5] fp32, labels int64 [R], loc_targets, loc_weights fp32 [R, 4*num_classes] (scda_proposal_finalize_hip)"""
    _req(cand_rois, "cand_rois"); _req(sel, "sel", torch.int32); _req(gt_of, "gt_of", torch.int32); _req(enc, "enc"); _req(gts, "gts")
    R, dev = sel.numel(), gts.device
    rois = torch.empty(R, 5, dtype=torch.float32, device=dev)
    labels = torch.empty(R, dtype=torch.int64, device=dev)
    t = torch.empty(R, 4 * num_classes, dtype=torch.float32, device=dev)
    w = torch.empty(R, 4 * num_classes, dtype=torch.float32, device=dev)
    _check(lib().scda_proposal_finalize_hip(_p(cand_rois), _p(sel), _p(gt_of), _p(enc), _p(gts), gts.shape[1], R, num_classes, image_index,
                                            _p(rois), _p(labels), _p(t), _p(w), _stream()), "scda_proposal_finalize_hip")
    return rois, labels, t, w


# ------------------------------------- cluster-region generator (cluster_ops.hip) ----
def kmeans_capacity():
    """most points one scda_kmeans_hip launch clusters (k <= 8)"""
    return lib().scda_kmeans_capacity()


def kmeans(rois, k, first_index, uniforms, bufs):
    """rois [N, >=5] fp32 rows (b, x1, y1, x2, y2, ..) on the device; first_index / uniforms: the seeding constants of (N, k) (a ctypes
    double array [k-1][t], or None for k = 1); bufs: caller-owned device buffers centres f32 [k,2], labels i32 [N], counts i32 [k],
    members i32 [k,N], seed_index i32 [k], n_iter i32 [1], status i32 [1] (scda_kmeans_hip: the rule is stated in include/scda_ops.h).
    One launch on the current stream; the caller reads status."""
    _req(rois, "rois")
    if rois.dim() != 2 or rois.shape[1] < 5 or k < 1:
        raise ValueError("kmeans: rois must be [N, >=5] and k >= 1")
    N = rois.shape[0]
    i32 = torch.int32
    _req_all("kmeans", ((bufs["centres"], "centres", torch.float32, 2 * k), (bufs["labels"], "labels", i32, N), (bufs["counts"], "counts", i32, k),
                        (bufs["members"], "members", i32, k * N), (bufs["seed_index"], "seed_index", i32, k), (bufs["n_iter"], "n_iter", i32, 1),
                        (bufs["status"], "status", i32, 1)))
    if any(b.device != rois.device for b in bufs.values()):
        raise ValueError("kmeans: every buffer must live on the device of rois")
    if k >= 2 and (uniforms is None or len(uniforms) < k - 1):
        raise ValueError("kmeans: uniforms must hold [k-1][t] draws")
    trials = 0 if uniforms is None or k < 2 else len(uniforms) // (k - 1)
    _check(lib().scda_kmeans_hip(_p(rois), rois.shape[1], N, k, first_index, uniforms, max(trials, 1), _p(bufs["centres"]), _p(bufs["labels"]),
                                 _p(bufs["counts"]), _p(bufs["members"]), _p(bufs["seed_index"]), _p(bufs["n_iter"]), _p(bufs["status"]),
                                 _stream()), "scda_kmeans_hip")


def cluster_gather(feats, members, counts, picks, k, threshold, out=None):
    """feats [N,F] fp32 (rows may be strided), members i32 [k,N], counts i32 [k], picks i32 [k, threshold] or None
    -> out fp32 [k, threshold, F]: the rows the cluster-region generator selects (scda_cluster_gather_hip)"""
    if not (isinstance(feats, torch.Tensor) and feats.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2 and feats.stride(1) == 1):
        raise ScdaNativeError("cluster_gather: feats must be a float32 [N,F] tensor on the HIP device with contiguous rows")
    _req(members, "members", torch.int32); _req(counts, "counts", torch.int32)
    if picks is not None:
        _req(picks, "picks", torch.int32)
        if picks.numel() != k * threshold:
            raise ValueError("cluster_gather: picks must be [k, threshold]")
    N, F = feats.shape
    if members.numel() != k * N or counts.numel() < k:
        raise ValueError("cluster_gather: members must be [k, N] and counts [k]")
    if out is None:
        out = torch.empty(k, threshold, F, dtype=torch.float32, device=feats.device)
    else:
        _req(out, "out")
        if out.numel() != k * threshold * F:
            raise ValueError("cluster_gather: out must be [k, threshold, F]")
    _check(lib().scda_cluster_gather_hip(_p(feats), feats.stride(0), N, F, _p(members), _p(counts), _p(picks), k, threshold, _p(out), _stream()),
           "scda_cluster_gather_hip")
    return out


def proposals_from_ranking(order, exp_wh, anchors64, loc, prob, A, fh, fw, img_h, img_w, min_size, nms_thresh, max_keep, image_index):
    """order int32 [n], exp_wh f32 [n,2] (device) -> (out6 fp32 [rows,6], num int64 [1]) on the device: decode + clip + size test,
    NMS, gather"""
    _req(order, "order", torch.int32); _req(exp_wh, "exp_wh"); _req(loc, "loc"); _req(prob, "prob")
    n = order.numel()
    dev = loc.device
    rows = max_keep if max_keep > 0 else max(n, 1)
    out6 = torch.zeros(rows, 6, dtype=torch.float32, device=dev)
    num = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return out6, num
    props = torch.empty(n, 5, dtype=torch.float32, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    L = lib()
    _check(L.scda_proposal_decode_hip(_p(order), _p(exp_wh), n, _p(anchors64), _p(loc), _p(prob), A, fh, fw, img_h, img_w, min_size,
                                      _p(props), _p(ok), _stream()), "scda_proposal_decode_hip")
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(max(L.scda_nms_workspace_bytes(n), 8), dtype=torch.uint8, device=dev)
    _check(L.scda_nms_valid_hip(_p(props), _p(ok), n, nms_thresh, _p(ws), _p(keep), _p(num), max_keep, _stream()), "scda_nms_valid_hip")
    _check(L.scda_proposal_gather_hip(_p(props), _p(keep), _p(num), image_index, rows, _p(out6), _stream()), "scda_proposal_gather_hip")
    return out6, num


# ------------------------------------------------ batched inference (infer_ops.hip) -------
def rpn_topk(prob, top_n, order=None, ws=None):
    """prob [B,2A,fh,fw] fp32 (soft-maxed) -> order int32 [B,n]: per image the anchor indices (flat (h, w, a) order) of the n best fg
    scores, score descending, ties by ascending index; n = top_n, or every anchor when top_n <= 0 or >= KA"""
    _req(prob, "prob")
    B, A2, fh, fw = prob.shape
    A = A2 // 2
    KA = A * fh * fw
    n = KA if top_n <= 0 or top_n >= KA else top_n
    L = lib()
    if order is None:
        order = torch.empty(B, n, dtype=torch.int32, device=prob.device)
    _req(order, "order", torch.int32)
    if ws is None:
        ws = torch.empty(max(L.scda_rpn_topk_workspace_bytes(B, KA, top_n), 8), dtype=torch.uint8, device=prob.device)
    _check(L.scda_rpn_topk_hip(_p(prob), B, A, fh, fw, top_n, _p(order), _p(ws), _stream()), "scda_rpn_topk_hip")
    return order


def rpn_proposals_workspace_bytes(B, A, fh, fw, top_n):
    return int(lib().scda_rpn_proposals_workspace_bytes(B, A, fh, fw, top_n))


def rpn_proposals_batched(prob, loc, anchors64, image_info, pre_nms_top_n, min_size, nms_thresh, post_nms_top_n, ws, rois5, props6,
                          counts):
    """functions/rpn_proposal.py for B images on the device, into the caller's fixed-capacity buffers: rois5 [B*P,5], props6 [B*P,6],
    counts int32 [B]; ws uint8 of rpn_proposals_workspace_bytes(...) bytes"""
    _req(prob, "prob"); _req(loc, "loc"); _req(anchors64, "anchors64", torch.float64); _req(image_info, "image_info")
    _req(ws, "ws", torch.uint8); _req(rois5, "rois5"); _req(props6, "props6"); _req(counts, "counts", torch.int32)
    B, A4, fh, fw = loc.shape
    A = A4 // 4
    P = int(post_nms_top_n)
    if tuple(prob.shape) != (B, 2 * A, fh, fw) or rois5.shape != (B * P, 5) or props6.shape != (B * P, 6) or counts.numel() != B:
        raise ValueError("rpn_proposals_batched: inconsistent shapes")
    if ws.numel() < rpn_proposals_workspace_bytes(B, A, fh, fw, pre_nms_top_n):
        raise ValueError("rpn_proposals_batched: workspace too small")
    _check(lib().scda_rpn_proposals_hip(_p(prob), _p(loc), _p(anchors64), B, A, fh, fw, _p(image_info), image_info.shape[1], pre_nms_top_n,
                                        min_size, nms_thresh, P, _p(ws), _p(rois5), _p(props6), _p(counts), _stream()),
           "scda_rpn_proposals_hip")
    return rois5, props6, counts


def box_predict_workspace_bytes(B, P, C):
    return int(lib().scda_box_predict_workspace_bytes(B, P, C))


def box_predict(rois, roi_counts, prob, loc, image_info, stds, means, score_thresh, nms_thresh, top_n, ws, det, det_counts, soft_nms=None):
    """functions/predict_bbox.py for B images on the device: rois [B*P,5] with roi_counts int32 [B] real rows per image, prob [B*P,C],
    loc [B*P,4C] -> det [B,top_n,7] (b, x1, y1, x2, y2, score, class), det_counts int32 [B] (the caller's buffers).
    soft_nms: None = hard NMS at nms_thresh; a setting (soft_nms_setting's dict, or its tuple) = the soft sweep in its place
    (scda_box_predict_soft_hip: nms_thresh plays no part, the top_n ranks by the rescored scores; P <= soft_nms_capacity())"""
    B = roi_counts.numel()
    R, C = prob.shape
    P = R // B
    if soft_nms is not None:                        # the setting and the capacity first: a wrong one is the caller's, whatever the device
        soft_nms = soft_nms if isinstance(soft_nms, tuple) else soft_nms_setting(soft_nms)
        if P > soft_nms_capacity():
            raise ValueError("box_predict: soft_nms holds a list of at most %d rows, P is %d" % (soft_nms_capacity(), P))
    _req(rois, "rois"); _req(roi_counts, "roi_counts", torch.int32); _req(prob, "prob"); _req(loc, "loc")
    _req(image_info, "image_info"); _req(ws, "ws", torch.uint8); _req(det, "det"); _req(det_counts, "det_counts", torch.int32)
    if P * B != R or rois.shape != (R, 5) or loc.shape != (R, 4 * C) or det.shape != (B, top_n, 7) or det_counts.numel() != B:
        raise ValueError("box_predict: inconsistent shapes")
    if ws.numel() < box_predict_workspace_bytes(B, P, C):
        raise ValueError("box_predict: workspace too small")
    s4, m4 = (ctypes.c_double * 4)(*[float(v) for v in stds]), (ctypes.c_double * 4)(*[float(v) for v in means])
    if soft_nms is not None:
        method, sigma, Nt, threshold = soft_nms
        _check(lib().scda_box_predict_soft_hip(_p(rois), _p(roi_counts), B, P, _p(prob), _p(loc), C, _p(image_info), image_info.shape[1],
                                               s4, m4, score_thresh, top_n, method, sigma, Nt, threshold, _p(ws), _p(det), _p(det_counts),
                                               _stream()), "scda_box_predict_soft_hip")
        return det, det_counts
    _check(lib().scda_box_predict_hip(_p(rois), _p(roi_counts), B, P, _p(prob), _p(loc), C, _p(image_info), image_info.shape[1], s4, m4,
                                      score_thresh, nms_thresh, top_n, _p(ws), _p(det), _p(det_counts), _stream()), "scda_box_predict_hip")
    return det, det_counts


# ------------------------------------------------- instance masks ------------
def det_rois(det, det_counts, rois5=None, cls=None):
    """det [B, top_n, 7] + det_counts int32 [B] (box_predict's outputs) -> rois5 [B*top_n, 5], cls int32 [B*top_n]; padding rows are
    (b, 0, 0, 0, 0), class -1"""
    _req(det, "det"); _req(det_counts, "det_counts", torch.int32)
    if det.dim() != 3 or det.shape[2] != 7 or det_counts.numel() != det.shape[0]:
        raise ValueError("det_rois: det must be [B, top_n, 7] and det_counts [B]")
    B, top_n = det.shape[:2]
    if rois5 is None:
        rois5 = torch.empty(B * top_n, 5, dtype=torch.float32, device=det.device)
    if cls is None:
        cls = torch.empty(B * top_n, dtype=torch.int32, device=det.device)
    _req(rois5, "rois5"); _req(cls, "cls", torch.int32)
    if rois5.shape != (B * top_n, 5) or cls.numel() != B * top_n:
        raise ValueError("det_rois: inconsistent shapes")
    _check(lib().scda_det_rois_hip(_p(det), _p(det_counts), B, top_n, _p(rois5), _p(cls), _stream()), "scda_det_rois_hip")
    return rois5, cls


def mask_select(logits, cls, sigmoid=False, out=None):
    """logits [R, C, h, w] in any strided order (not required contiguous) + cls int32 [R] -> [R, h, w] contiguous: each row's own class
    plane, optionally through the sigmoid; rows of class < 0 give zeros"""
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype != torch.float32:
        raise ScdaNativeError("logits must be a float32 tensor on the HIP device; there is no CPU path")
    _req(cls, "cls", torch.int32)
    if logits.dim() != 4 or cls.numel() != logits.shape[0]:
        raise ValueError("mask_select: logits must be [R, C, h, w] and cls [R]")
    R, C, h, w = logits.shape
    if min(logits.stride()) < 0:
        raise ValueError("mask_select: negative strides")
    if out is None:
        out = torch.empty(R, h, w, dtype=torch.float32, device=logits.device)
    _req(out, "out")
    if out.shape != (R, h, w):
        raise ValueError("mask_select: out must be [R, h, w]")
    sr, sc, sh, sw = logits.stride()
    _check(lib().scda_mask_select_hip(_p(logits), sr, sc, sh, sw, _p(cls), R, C, h, w, 1 if sigmoid else 0, _p(out), _stream()),
           "scda_mask_select_hip")
    return out


MASK_PLANE_MAX = 32


def _check_windows(who, rois, planes, ndim, what, noun, cls, max_side):
    """the common arguments of the kernels that resize a plane to its RoI window (dtypes and devices of rois and planes already
    checked): rois [R, >=5], planes [R, ..., h, w] of ndim axes with h, w <= max_side, cls None or int32 [R]"""
    if rois.dim() != 2 or rois.shape[1] < 5 or planes.dim() != ndim or planes.shape[0] != rois.shape[0]:
        raise ValueError("%s: rois must be [R, >=5] and %s" % (who, what))
    if max(planes.shape[-2:]) > max_side:
        raise ValueError("%s: %s of at most %d x %d" % (who, noun, max_side, max_side))
    if cls is not None:
        _req(cls, "cls", torch.int32)
        if cls.numel() != rois.shape[0]:
            raise ValueError("%s: cls must be [R]" % who)


def mask_paste(rois, planes, H, W, cls=None, packed=False, threshold=0.5, out=None):
    """functions/mask.py:21-49 on the device (include/scda_ops.h states the rule): rois [R, >=5] (b, x1, y1, x2, y2, ...), planes
    [R, h, w] -> float32 [R, H, W], or with packed=True uint32 [R, H, ceil(W/32)] of (value >= threshold), stored as int32.  Rows
    with cls < 0 give an empty mask; the part of a window outside the plane is dropped.  Every element of `out` is written."""
    _req(rois, "rois"); _req(planes, "planes")
    _check_windows("mask_paste", rois, planes, 3, "planes [R, h, w]", "planes", cls, MASK_PLANE_MAX)
    R, h, w = planes.shape
    H, W = int(H), int(W)
    shape, dtype = ((R, H, (W + 31) // 32), torch.int32) if packed else ((R, H, W), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=rois.device)
    _req(out, "out", dtype)
    if tuple(out.shape) != shape:
        raise ValueError("mask_paste: out must be %s" % (shape,))
    _check(lib().scda_mask_paste_hip(_p(rois), rois.shape[1], _p(cls), _p(planes), R, h, w, H, W, 1 if packed else 0, threshold, _p(out),
                                     _stream()), "scda_mask_paste_hip")
    return out


KEYPOINT_PLANE_MAX = 64


def keypoint_decode_workspace_bytes(R, Kp, W):
    return int(lib().scda_keypoint_decode_workspace_bytes(int(R), int(Kp), int(W)))


def keypoint_decode(rois, heat, H, W, cls=None, out=None, ws=None):
    """R x Kp heat maps -> float32 [R, Kp, 3] rows (x, y, score) on the device (include/scda_ops.h states the rule: each heat map resized
    to its RoI as functions/mask.py:21-49 resizes a mask plane, then np.argmax over the part of the window inside (H, W); the choice
    of rule is ours, its parity is pinned to predict_masks + np.argmax).  rois [R, >=5] (b, x1, y1, x2, y2, ...), heat [R, Kp, h, w]
    in any strided order (not required contiguous), h, w <= 64; cls int32 [R]: rows with cls < 0 (padding) give (0, 0, 0), as do empty
    or non-finite windows and windows wholly outside (H, W).  ws: a uint8 buffer of keypoint_decode_workspace_bytes(R, Kp, W)."""
    _req(rois, "rois")
    if not isinstance(heat, torch.Tensor) or not heat.is_cuda or heat.dtype != torch.float32:
        raise ScdaNativeError("heat must be a float32 tensor on the HIP device; there is no CPU path")
    _check_windows("keypoint_decode", rois, heat, 4, "heat [R, Kp, h, w]", "heat maps", cls, KEYPOINT_PLANE_MAX)
    R, Kp, h, w = heat.shape
    if min(heat.stride()) < 0:
        raise ValueError("keypoint_decode: negative strides")
    H, W = int(H), int(W)
    if out is None:
        out = torch.empty(R, Kp, 3, dtype=torch.float32, device=rois.device)
    _req(out, "out")
    if tuple(out.shape) != (R, Kp, 3):
        raise ValueError("keypoint_decode: out must be [R, Kp, 3]")
    need = keypoint_decode_workspace_bytes(R, Kp, W)
    if ws is None:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=rois.device)
    _req(ws, "ws", torch.uint8)
    if ws.numel() < need:
        raise ValueError("keypoint_decode: ws holds %d bytes, %d needed" % (ws.numel(), need))
    sr, sk, sh, sw = heat.stride()
    _check(lib().scda_keypoint_decode_hip(_p(rois), rois.shape[1], _p(cls), _p(heat), sr, sk, sh, sw, R, Kp, h, w, H, W, _p(ws), _p(out),
                                          _stream()), "scda_keypoint_decode_hip")
    return out


def _keypoint_planes(who, heat, name="heat"):
    """heat float32 [R, Kp, h, w] on the device whose (h, w) planes are contiguous, R and Kp strided at will -> (R, Kp, HW, sr, sk)"""
    if not isinstance(heat, torch.Tensor) or not heat.is_cuda or heat.dtype != torch.float32:
        raise ScdaNativeError(f"{who}: {name} must be a float32 tensor on the HIP device; there is no CPU path")
    if heat.dim() != 4 or heat.numel() == 0:
        raise ValueError(f"{who}: {name} must be a non-empty [R, Kp, h, w]")
    R, Kp, h, w = heat.shape
    if h * w > KEYPOINT_PLANE_MAX * KEYPOINT_PLANE_MAX:
        raise ValueError(f"{who}: maps of {h} x {w} = {h * w} elements; the kernel holds at most "
                         f"{KEYPOINT_PLANE_MAX * KEYPOINT_PLANE_MAX} ({KEYPOINT_PLANE_MAX} x {KEYPOINT_PLANE_MAX}, the decode's limit)")
    sr, sk, sh, sw = heat.stride()
    if (w > 1 and sw != 1) or (h > 1 and sh != w) or sr < 0 or sk < 0:
        raise ValueError(f"{who}: every (h, w) plane of {name} must be contiguous (strides {tuple(heat.stride())})")
    return R, Kp, h * w, sr, sk


def keypoint_ce_fwd(heat, targets, stats=None, row_loss=None):
    """The keypoint heat-map loss (include/scda_ops.h states it): heat [R, Kp, h, w] -- contiguous, or the keypoint head's transposed
    channel-major view, taken as it is --, targets int32 [R, Kp] (-1: not counted) -> (out2 = (mean over the counted pairs of
    logsumexp(map) - map[target], their number), stats [R * Kp, 2] for the backward, row_loss [R * Kp]).  stats, row_loss: optional
    buffers of those shapes to fill."""
    R, Kp, HW, sr, sk = _keypoint_planes("keypoint_ce_fwd", heat)
    _req(targets, "targets", torch.int32)
    if tuple(targets.shape) != (R, Kp):
        raise ValueError("keypoint_ce_fwd: targets must be [R, Kp] = [%d, %d], got %s" % (R, Kp, tuple(targets.shape)))
    if stats is None:
        stats = torch.empty(R * Kp, 2, dtype=torch.float32, device=heat.device)
    if row_loss is None:
        row_loss = torch.empty(R * Kp, dtype=torch.float32, device=heat.device)
    _req(stats, "stats"); _req(row_loss, "row_loss")
    if tuple(stats.shape) != (R * Kp, 2) or tuple(row_loss.shape) != (R * Kp,):
        raise ValueError("keypoint_ce_fwd: stats must be [R * Kp, 2] and row_loss [R * Kp]")
    out2 = torch.empty(2, dtype=torch.float32, device=heat.device)
    _check(lib().scda_keypoint_ce_fwd_hip(_p(heat), sr, sk, R, Kp, HW, _p(targets), _p(stats), _p(row_loss), _p(out2), _stream()),
           "scda_keypoint_ce_fwd_hip")
    return out2, stats, row_loss


def keypoint_ce_bwd(heat, targets, stats, out2, g, out=None):
    """-> d loss / d heat in heat's own layout (a tensor of heat's shape and strides): (softmax - onehot) * g / count on counted maps,
    exactly zero on the others.  g: one float32 on the device.  out: a tensor of heat's shape with contiguous planes to fill."""
    R, Kp, HW, sr, sk = _keypoint_planes("keypoint_ce_bwd", heat)
    _req(g, "g"); _req(targets, "targets", torch.int32); _req(stats, "stats"); _req(out2, "out2")
    if targets.numel() != R * Kp or stats.numel() != 2 * R * Kp or out2.numel() != 2 or g.numel() != 1:
        raise ValueError("keypoint_ce_bwd: targets [R, Kp], stats [R * Kp, 2], out2 [2] and g [1] of the forward call are needed")
    if out is None:
        out = torch.empty_like(heat)          # (preserve_format: heat's strides when it is dense, its dimension order otherwise)
    if tuple(out.shape) != tuple(heat.shape):
        raise ValueError("keypoint_ce_bwd: out must have heat's shape")
    _, _, _, dsr, dsk = _keypoint_planes("keypoint_ce_bwd", out, "out")
    _check(lib().scda_keypoint_ce_bwd_hip(_p(heat), sr, sk, R, Kp, HW, _p(targets), _p(stats), _p(out2), _p(g), _p(out), dsr, dsk,
                                          _stream()), "scda_keypoint_ce_bwd_hip")
    return out


def mask_rescale_max_ratio():
    """the largest down-scale h / oh, w / ow of mask_rescale (a capacity of the kernel's LDS tables)"""
    return int(lib().scda_mask_rescale_max_ratio())


def mask_rescale(rois, planes, H, W, image_info, Ho, Wo, cls=None, packed=False, threshold=0.5, out=None, foot_rois=None, status=None):
    """tools/mask_rcnn_train_val.py:422-423 on the device (include/scda_ops.h states the rule): rois [R, >=5], planes [R, h, w] as
    mask_paste takes them at the padded (H, W); image_info float32 [B, >=5] on the device, rows (h, w, resize_scale, origin_h, origin_w),
    R % B == 0 (detection r belongs to image r // (R // B)).  Each detection's pasted plane, cut to its image's (h, w), is resized to the
    image's (origin_h, origin_w) as Pillow does and written into planes of (Ho, Wo): float32 [R, Ho, Wo], or with packed=True uint32
    [R, Ho, ceil(Wo/32)] of (value > threshold), stored as int32.  -> (out, foot_rois float32 [R, 5] = (b, fx1, fy1, fx2, fy2), the
    rectangle outside which nothing was computed -- mask_rle's `rois` hint when threshold >= 0 --, status int32 [B], non-zero for an image
    beyond the limits, whose masks are empty).  Every element of the three is written.  No wait for the host."""
    _req(rois, "rois"); _req(planes, "planes"); _req(image_info, "image_info")
    _check_windows("mask_rescale", rois, planes, 3, "planes [R, h, w]", "planes", cls, MASK_PLANE_MAX)
    R, h, w = planes.shape
    if image_info.dim() != 2 or image_info.shape[1] < 5 or image_info.shape[0] < 1 or R % image_info.shape[0]:
        raise ValueError("mask_rescale: image_info must be [B, >=5] (h, w, resize_scale, origin_h, origin_w) with R a multiple of B")
    B = image_info.shape[0]
    H, W, Ho, Wo = int(H), int(W), int(Ho), int(Wo)
    if min(H, W, Ho, Wo) < 1:
        raise ValueError("mask_rescale: H, W, Ho, Wo must be >= 1")
    shape, dtype = ((R, Ho, (Wo + 31) // 32), torch.int32) if packed else ((R, Ho, Wo), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=rois.device)
    if foot_rois is None:
        foot_rois = torch.empty(R, 5, dtype=torch.float32, device=rois.device)
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=rois.device)
    _req(out, "out", dtype); _req(foot_rois, "foot_rois"); _req(status, "status", torch.int32)
    if tuple(out.shape) != shape or tuple(foot_rois.shape) != (R, 5) or status.numel() != B:
        raise ValueError("mask_rescale: out must be %s, foot_rois [R, 5] and status [B]" % (shape,))
    _check(lib().scda_mask_rescale_hip(_p(rois), rois.shape[1], _p(cls), _p(planes), R, h, w, H, W, _p(image_info), image_info.shape[1],
                                       R // B, Ho, Wo, 1 if packed else 0, threshold, _p(out), _p(foot_rois), _p(status), _stream()),
           "scda_mask_rescale_hip")
    return out, foot_rois, status


# ------------------------------------------------- COCO run-length results ---
def mask_rle_max_chars(h, w):
    """characters one count of an h x w plane can take in the 6-bit string: ceil((bitlength(h * w) + 1) / 5)"""
    return int(lib().scda_mask_rle_max_chars(int(h), int(w)))


def mask_rle_workspace_bytes(R, H, Wd, cap_runs):
    return int(lib().scda_mask_rle_workspace_bytes(R, H, Wd, cap_runs))


def _words(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ScdaNativeError(f"{name} must live on the HIP device; there is no CPU path")
    if t.dtype != torch.int32 or t.dim() != 3 or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous int32 [R, H, ceil(W/32)] words")
    return t


def mask_rle(bits, size=None, image_info=None, rois=None, cap_runs=None, ws=None, out=None, info_column=0):
    """maskApi.c's rleEncode / rleToString / rleArea / rleToBbox of packed masks on the device (include/scda_ops.h states the rules).
    bits int32 [R, H, Wd] words as mask_paste(packed=True) writes them.  The image of each mask: size=(h, w) for all, or image_info
    float32 [B, >=2] on the device with R % B == 0 (mask r belongs to image r // (R // B)); default: the whole plane.  rois [R, >=5]: the
    rows given to mask_paste, a hint that limits the columns read (planes pasted with threshold > 0 only).  cap_runs: runs kept per mask
    (default 4 * 32 * Wd).  -> dict of device tensors n_runs int32 [R] (the true count; > cap_runs = overflow), counts int32 [R, cap_runs]
    (uint32 values), n_bytes int32 [R], chars uint8 [R, cap_runs * mask_rle_max_chars(H, 32 Wd)], area int32 [R], bbox int32 [R, 4]
    (x, y, w, h).  ws / out: buffers of an earlier call of the same shape, reused.  No wait for the host.
    info_column: the column of image_info where (h, w) stand -- 3 reads the (origin_h, origin_w) of the loader's rows, for planes that
    mask_rescale wrote."""
    _words(bits, "bits")
    R, H, Wd = bits.shape
    cap_runs = 4 * 32 * Wd if cap_runs is None else int(cap_runs)
    if cap_runs < 1:
        raise ValueError("mask_rle: cap_runs must be >= 1")
    cap_bytes = cap_runs * mask_rle_max_chars(H, 32 * Wd)
    h_all = w_all = per = stride = 0
    if image_info is not None:
        if size is not None:
            raise ValueError("mask_rle: give size or image_info, not both")
        _req(image_info, "image_info")
        info_column = int(info_column)
        if image_info.dim() != 2 or info_column < 0 or image_info.shape[1] < info_column + 2 or R % image_info.shape[0]:
            raise ValueError("mask_rle: image_info must be [B, >= info_column + 2] with R a multiple of B")
        per, stride = R // image_info.shape[0], image_info.shape[1]
    else:
        h_all, w_all = (H, 32 * Wd) if size is None else (int(size[0]), int(size[1]))
        if not (1 <= h_all <= H and 1 <= w_all <= 32 * Wd):
            raise ValueError("mask_rle: size must lie in [1, %d] x [1, %d]" % (H, 32 * Wd))
    rstride = 0
    if rois is not None:
        _req(rois, "rois")
        if rois.dim() != 2 or rois.shape[0] != R or rois.shape[1] < 5:
            raise ValueError("mask_rle: rois must be [R, >=5]")
        rstride = rois.shape[1]
    need = mask_rle_workspace_bytes(R, H, Wd, cap_runs)
    if need == 0:
        raise ValueError("mask_rle: planes of at most 65535 masks x 65535 rows and fewer than 2^31 pixels")
    dev = bits.device
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _req(ws, "ws", torch.uint8)
    if ws.numel() < need:
        raise ValueError("mask_rle: workspace too small")
    if out is None:
        i = dict(dtype=torch.int32, device=dev)
        out = {'n_runs': torch.empty(R, **i), 'counts': torch.empty(R, cap_runs, **i), 'n_bytes': torch.empty(R, **i),
               'chars': torch.empty(R, cap_bytes, dtype=torch.uint8, device=dev), 'area': torch.empty(R, **i),
               'bbox': torch.empty(R, 4, **i)}
    for k, shape, dt in (('n_runs', (R,), torch.int32), ('counts', (R, cap_runs), torch.int32), ('n_bytes', (R,), torch.int32),
                         ('chars', (R, cap_bytes), torch.uint8), ('area', (R,), torch.int32), ('bbox', (R, 4), torch.int32)):
        _req(out[k], k, dt)
        if out[k].numel() != R * (shape[1] if len(shape) > 1 else 1):
            raise ValueError("mask_rle: out[%r] must hold %s" % (k, shape))
    info_ptr = None if image_info is None else image_info.data_ptr() + 4 * info_column
    _check(lib().scda_mask_rle_hip(_p(bits), R, H, Wd, info_ptr, stride, per, h_all, w_all, _p(rois), rstride, cap_runs, cap_bytes,
                                   _p(ws), _p(out['n_runs']), _p(out['counts']), _p(out['n_bytes']), _p(out['chars']), _p(out['area']),
                                   _p(out['bbox']), _stream()), "scda_mask_rle_hip")
    return out


def mask_iou_workspace_bytes(M, N, H, Wd):
    return int(lib().scda_mask_iou_workspace_bytes(M, N, H, Wd))


def mask_iou(dt_bits, gt_bits, size, iscrowd=None, ws=None, out=None):
    """maskApi.c's rleIou of packed masks on the device: dt_bits int32 [M, H, Wd], gt_bits int32 [N, H, Wd], size = (h, w) of the image
    inside the planes, iscrowd uint8 [N] on the device or None -> (iou float64 [N, M], inter int32 [N, M] holding uint32 counts); the
    box gate of the reference included (include/scda_ops.h).  ws (uint8, mask_iou_workspace_bytes) / out = (iou, inter): buffers of the
    caller, so that nothing is allocated."""
    _words(dt_bits, "dt_bits"); _words(gt_bits, "gt_bits")
    M, H, Wd = dt_bits.shape
    N = gt_bits.shape[0]
    if tuple(gt_bits.shape[1:]) != (H, Wd) or M < 1 or N < 1:
        raise ValueError("mask_iou: dt_bits [M, H, Wd] and gt_bits [N, H, Wd] with M, N >= 1")
    h, w = int(size[0]), int(size[1])
    if not (1 <= h <= H and 1 <= w <= 32 * Wd):
        raise ValueError("mask_iou: size must lie in [1, %d] x [1, %d]" % (H, 32 * Wd))
    if iscrowd is not None:
        _req(iscrowd, "iscrowd", torch.uint8)
        if iscrowd.numel() != N:
            raise ValueError("mask_iou: iscrowd must be [N]")
    need = int(lib().scda_mask_iou_workspace_bytes(M, N, H, Wd))
    if need == 0:
        raise ValueError("mask_iou: planes of at most 65535 masks x 65535 rows and fewer than 2^31 pixels")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dt_bits.device)
    _req(ws, "ws", torch.uint8)
    if ws.numel() < need:
        raise ValueError("mask_iou: workspace too small")
    if out is None:
        out = (torch.empty(N, M, dtype=torch.float64, device=dt_bits.device),
               torch.empty(N, M, dtype=torch.int32, device=dt_bits.device))
    iou, inter = _req(out[0], "iou", torch.float64), _req(out[1], "inter", torch.int32)
    if iou.numel() != N * M or inter.numel() != N * M:
        raise ValueError("mask_iou: out must hold [N, M]")
    _check(lib().scda_mask_iou_hip(_p(dt_bits), M, _p(gt_bits), N, H, Wd, h, w, _p(iscrowd), _p(ws), _p(iou), _p(inter), _stream()),
           "scda_mask_iou_hip")
    return iou, inter


# ------------------------------------- COCO ground-truth masks (annToMask) ---
def mask_frpoly_workspace_bytes(P, Q, H, Wd):
    return int(lib().scda_mask_frpoly_workspace_bytes(int(P), int(Q), int(H), int(Wd)))


def mask_frpoly(xy, poly_first, poly_plane, rle_counts, rle_first, rle_plane, sizes, ws, out, area=None):
    """COCO.annToMask on the device (include/scda_ops.h states the rule): polygons xy float64 [V, 2], poly_first int32 [P + 1], poly_plane
    int32 [P]; run lengths rle_counts int32 [C] (uint32 values), rle_first int32 [Q + 1], rle_plane int32 [Q]; sizes int32 [N, 2] = (h, w)
    of the image inside plane n -- all device tensors as scda_amd.coco_gt.flatten_annotations lays them out (it also checks the limits on
    the data, which this wrapper cannot see).  ws: uint8, mask_frpoly_workspace_bytes(P, Q, H, Wd); out: int32 [N, H, Wd] words, every one
    of which is written; area: int32 [N] (uint32 values) or None.  Nothing is allocated and the host is not waited for.  -> out"""
    _req(xy, "xy", torch.float64); _req(sizes, "sizes", torch.int32); _req(ws, "ws", torch.uint8)
    for t, name in ((poly_first, "poly_first"), (poly_plane, "poly_plane"), (rle_counts, "rle_counts"), (rle_first, "rle_first"),
                    (rle_plane, "rle_plane")):
        _req(t, name, torch.int32)
    _words(out, "out")
    N, H, Wd = out.shape
    V, P, C, Q = xy.shape[0], poly_plane.numel(), rle_counts.numel(), rle_plane.numel()
    if xy.dim() != 2 or xy.shape[1] != 2 or poly_first.numel() != P + 1 or rle_first.numel() != Q + 1 or tuple(sizes.shape) != (N, 2):
        raise ValueError("mask_frpoly: xy [V, 2], poly_first [P + 1], poly_plane [P], rle_first [Q + 1], rle_plane [Q], sizes [N, 2]")
    need = mask_frpoly_workspace_bytes(P, Q, H, Wd)
    if need == 0 or not (1 <= N <= 65535):
        raise ValueError("mask_frpoly: at most 65535 planes x 65535 rows and fewer than 2^31 pixels")
    if ws.numel() < need:
        raise ValueError("mask_frpoly: workspace too small")
    if area is not None:
        _req(area, "area", torch.int32)
        if area.numel() != N:
            raise ValueError("mask_frpoly: area must be [N]")
    _check(lib().scda_mask_frpoly_hip(_p(xy), V, _p(poly_first), _p(poly_plane), P, _p(rle_counts), C, _p(rle_first), _p(rle_plane), Q,
                                      _p(sizes), N, H, Wd, _p(ws), _p(out), _p(area), _stream()), "scda_mask_frpoly_hip")
    return out


# ------------------------------------------------- COCO AP (COCOeval) -------
def _req_all(what, specs):
    for t, name, dt, n in specs:
        _req(t, name, dt)
        if t.numel() < n:
            raise ValueError(f"{what}: {name} holds {t.numel()} elements, {n} needed")


def coco_det_rows(detections, detection_counts, K, xywh, area, score, cat, mask_area=None):
    """detections float32 [B, top_n, 7] + detection_counts int32 [B] -> the caller's xywh float64 [B, top_n, 4], area float64, score
    float32, cat int32 [B, top_n] (include/scda_ops.h: scda_coco_det_rows_hip).  mask_area int32 [B, top_n]: the RLE area, for 'segm'."""
    _req(detections, "detections"); _req(detection_counts, "detection_counts", torch.int32)
    if detections.dim() != 3 or detections.shape[2] != 7 or detection_counts.numel() != detections.shape[0]:
        raise ValueError("coco_det_rows: detections [B, top_n, 7] and detection_counts [B]")
    B, top_n = detections.shape[:2]
    for t, name, dt, n in ((xywh, "xywh", torch.float64, 4), (area, "area", torch.float64, 1), (score, "score", torch.float32, 1),
                           (cat, "cat", torch.int32, 1)):
        _req(t, name, dt)
        if t.numel() != B * top_n * n:
            raise ValueError(f"coco_det_rows: {name} must hold [B, top_n{', 4' if n == 4 else ''}]")
    if mask_area is not None:
        _req(mask_area, "mask_area", torch.int32)
        if mask_area.numel() != B * top_n:
            raise ValueError("coco_det_rows: mask_area must be [B, top_n]")
    _check(lib().scda_coco_det_rows_hip(_p(detections), _p(detection_counts), B, top_n, _p(mask_area), int(K), _p(xywh), _p(area),
                                        _p(score), _p(cat), _stream()), "scda_coco_det_rows_hip")


def coco_box_iou(dt, dt_counts, gt, gt_counts, iscrowd, out=None):
    """bbIou for B images: dt float64 [B, D, 4], gt float64 [B, G, 4] (x, y, w, h), iscrowd uint8 [B, G], counts int32 [B] -> iou float64
    [B, G, D] (o[g * D + d] per image), written where d < dt_counts[b] and g < gt_counts[b]; a fresh `out` is zero elsewhere"""
    _req(dt, "dt", torch.float64); _req(gt, "gt", torch.float64); _req(iscrowd, "iscrowd", torch.uint8)
    _req(dt_counts, "dt_counts", torch.int32); _req(gt_counts, "gt_counts", torch.int32)
    if dt.dim() != 3 or gt.dim() != 3 or dt.shape[2] != 4 or gt.shape[2] != 4 or gt.shape[0] != dt.shape[0]:
        raise ValueError("coco_box_iou: dt [B, D, 4] and gt [B, G, 4]")
    B, D, G = dt.shape[0], dt.shape[1], gt.shape[1]
    if iscrowd.numel() != B * G or dt_counts.numel() != B or gt_counts.numel() != B:
        raise ValueError("coco_box_iou: iscrowd [B, G], counts [B]")
    if not (1 <= D <= 1024 and 1 <= G <= 1024):
        raise ValueError("coco_box_iou: 1 <= D, G <= 1024")
    if out is None:
        out = torch.zeros(B, G, D, dtype=torch.float64, device=dt.device)
    _req(out, "out", torch.float64)
    if out.numel() < B * G * D:
        raise ValueError("coco_box_iou: out must hold [B, G, D]")
    _check(lib().scda_coco_box_iou_hip(_p(dt), _p(dt_counts), _p(gt), _p(gt_counts), _p(iscrowd), B, D, G, _p(out), _stream()),
           "scda_coco_box_iou_hip")
    return out


def _coco_rows_out(what, B, top_n, xywh, area, score, cat):
    for t, name, dt, n in ((xywh, "xywh", torch.float64, 4), (area, "area", torch.float64, 1), (score, "score", torch.float32, 1),
                           (cat, "cat", torch.int32, 1)):
        _req(t, name, dt)
        if t.numel() != B * top_n * n:
            raise ValueError(f"{what}: {name} must hold [B, top_n{', 4' if n == 4 else ''}]")


def coco_kp_rows(detections, detection_counts, keypoints, K, xywh, area, score, cat):
    """coco_det_rows for keypoint results: detections float32 [B, top_n, 7] give score and class, keypoints float32 [B, top_n, Kp, 3]
    the box and area (include/scda_ops.h: scda_coco_kp_rows_hip)"""
    _req(detections, "detections"); _req(detection_counts, "detection_counts", torch.int32); _req(keypoints, "keypoints")
    if detections.dim() != 3 or detections.shape[2] != 7 or detection_counts.numel() != detections.shape[0]:
        raise ValueError("coco_kp_rows: detections [B, top_n, 7] and detection_counts [B]")
    B, top_n = detections.shape[:2]
    if keypoints.dim() != 4 or tuple(keypoints.shape[:2]) != (B, top_n) or keypoints.shape[3] != 3 or not 1 <= keypoints.shape[2] <= 32:
        raise ValueError("coco_kp_rows: keypoints [B, top_n, Kp, 3], 1 <= Kp <= 32")
    _coco_rows_out("coco_kp_rows", B, top_n, xywh, area, score, cat)
    _check(lib().scda_coco_kp_rows_hip(_p(detections), _p(detection_counts), B, top_n, _p(keypoints), int(keypoints.shape[2]), int(K),
                                       _p(xywh), _p(area), _p(score), _p(cat), _stream()), "scda_coco_kp_rows_hip")


def coco_prop_rows(proposals, proposal_counts, xywh, area, score, cat, xyxy_as_xywh=False):
    """coco_det_rows from proposals float32 [B, P, 6] = (b, x1, y1, x2, y2, score) + proposal_counts int32 [B], category 1
    (include/scda_ops.h: scda_coco_prop_rows_hip); xyxy_as_xywh: the reference's 'proposal' rows, (x2, y2) taken as (w, h)"""
    _req(proposals, "proposals"); _req(proposal_counts, "proposal_counts", torch.int32)
    if proposals.dim() != 3 or proposals.shape[2] != 6 or proposal_counts.numel() != proposals.shape[0]:
        raise ValueError("coco_prop_rows: proposals [B, P, 6] and proposal_counts [B]")
    B, P = proposals.shape[:2]
    _coco_rows_out("coco_prop_rows", B, P, xywh, area, score, cat)
    _check(lib().scda_coco_prop_rows_hip(_p(proposals), _p(proposal_counts), B, P, int(bool(xyxy_as_xywh)), _p(xywh), _p(area), _p(score),
                                         _p(cat), _stream()), "scda_coco_prop_rows_hip")


def coco_oks(dt_keypoints, dt_counts, gt_keypoints, gt_boxes, gt_areas, gt_counts, vars_, out=None, gt_iscrowd=None,
             gt_num_keypoints=None, gt_ignore=None):
    """computeOks for B images: dt_keypoints float32 [B, D, Kp, 3], gt_keypoints float64 [B, G, Kp, 3], gt_boxes float64 [B, G, 4],
    gt_areas float64 [B, G], counts int32 [B], vars_ float64 [Kp] -> oks float64 [B, G, D], written where d < dt_counts[b] and
    g < gt_counts[b]; a fresh `out` is zero elsewhere.  gt_ignore uint8 [B, G] (with gt_iscrowd uint8 and gt_num_keypoints int32 [B, G]):
    also iscrowd || num_keypoints == 0 per live GT (include/scda_ops.h: scda_coco_oks_hip)"""
    _req(dt_keypoints, "dt_keypoints"); _req(gt_keypoints, "gt_keypoints", torch.float64); _req(gt_boxes, "gt_boxes", torch.float64)
    _req(gt_areas, "gt_areas", torch.float64); _req(vars_, "vars", torch.float64)
    _req(dt_counts, "dt_counts", torch.int32); _req(gt_counts, "gt_counts", torch.int32)
    if dt_keypoints.dim() != 4 or gt_keypoints.dim() != 4 or dt_keypoints.shape[3] != 3 or gt_keypoints.shape[3] != 3 or \
            gt_keypoints.shape[0] != dt_keypoints.shape[0] or gt_keypoints.shape[2] != dt_keypoints.shape[2]:
        raise ValueError("coco_oks: dt_keypoints [B, D, Kp, 3] and gt_keypoints [B, G, Kp, 3]")
    B, D, Kp = dt_keypoints.shape[:3]
    G = gt_keypoints.shape[1]
    if not (1 <= D <= 1024 and 1 <= G <= 1024 and 1 <= Kp <= 32):
        raise ValueError("coco_oks: 1 <= D, G <= 1024, 1 <= Kp <= 32")
    if gt_boxes.numel() != B * G * 4 or gt_areas.numel() != B * G or vars_.numel() != Kp or dt_counts.numel() != B or gt_counts.numel() != B:
        raise ValueError("coco_oks: gt_boxes [B, G, 4], gt_areas [B, G], vars [Kp], counts [B]")
    if gt_ignore is not None:
        if gt_iscrowd is None or gt_num_keypoints is None:
            raise ValueError("coco_oks: gt_ignore needs gt_iscrowd and gt_num_keypoints")
        _req(gt_ignore, "gt_ignore", torch.uint8); _req(gt_iscrowd, "gt_iscrowd", torch.uint8)
        _req(gt_num_keypoints, "gt_num_keypoints", torch.int32)
        if gt_ignore.numel() < B * G or gt_iscrowd.numel() != B * G or gt_num_keypoints.numel() != B * G:
            raise ValueError("coco_oks: gt_ignore, gt_iscrowd and gt_num_keypoints [B, G]")
    if out is None:
        out = torch.zeros(B, G, D, dtype=torch.float64, device=dt_keypoints.device)
    _req(out, "out", torch.float64)
    if out.numel() < B * G * D:
        raise ValueError("coco_oks: out must hold [B, G, D]")
    given = gt_ignore is not None
    _check(lib().scda_coco_oks_hip(_p(dt_keypoints), _p(dt_counts), _p(gt_keypoints), _p(gt_boxes), _p(gt_areas), _p(gt_counts), _p(vars_),
                                   Kp, _p(gt_iscrowd) if given else None, _p(gt_num_keypoints) if given else None, B, D, G, _p(out),
                                   _p(gt_ignore), _stream()), "scda_coco_oks_hip")
    return out


def coco_regroup(K, dt_counts, in_xywh, in_area, in_score, in_cat, gt_counts, gt_cat, gt_area, gt_iscrowd, in_iou, xywh, area, score, cat,
                 out_gt_area, out_gt_iscrowd, out_gt_cat, out_iou, perm_dets, perm_gts):
    """the useCats = 0 order made physical (include/scda_ops.h: scda_coco_regroup_hip): rows and IoU block of B images regrouped by
    (category ascending, given order); in_* [B, D(, 4)] and gt_* [B, G] are read, everything behind in_iou is written"""
    B, D = in_cat.shape
    G = gt_cat.shape[1]
    _req_all("coco_regroup", ((dt_counts, "dt_counts", torch.int32, B), (in_xywh, "in_xywh", torch.float64, B * D * 4),
                              (in_area, "in_area", torch.float64, B * D), (in_score, "in_score", torch.float32, B * D),
                              (in_cat, "in_cat", torch.int32, B * D), (gt_counts, "gt_counts", torch.int32, B),
                              (gt_cat, "gt_cat", torch.int32, B * G), (gt_area, "gt_area", torch.float64, B * G),
                              (gt_iscrowd, "gt_iscrowd", torch.uint8, B * G), (in_iou, "in_iou", torch.float64, B * G * D),
                              (xywh, "xywh", torch.float64, B * D * 4), (area, "area", torch.float64, B * D),
                              (score, "score", torch.float32, B * D), (cat, "cat", torch.int32, B * D),
                              (out_gt_area, "out_gt_area", torch.float64, B * G), (out_gt_iscrowd, "out_gt_iscrowd", torch.uint8, B * G),
                              (out_gt_cat, "out_gt_cat", torch.int32, B * G), (out_iou, "out_iou", torch.float64, B * G * D),
                              (perm_dets, "perm_dets", torch.int32, B * D), (perm_gts, "perm_gts", torch.int32, B * G)))
    _check(lib().scda_coco_regroup_hip(B, D, G, int(K), _p(dt_counts), _p(in_xywh), _p(in_area), _p(in_score), _p(in_cat), _p(gt_counts),
                                       _p(gt_cat), _p(gt_area), _p(gt_iscrowd), _p(in_iou), _p(xywh), _p(area), _p(score), _p(cat),
                                       _p(out_gt_area), _p(out_gt_iscrowd), _p(out_gt_cat), _p(out_iou), _p(perm_dets), _p(perm_gts),
                                       _stream()), "scda_coco_regroup_hip")


def coco_match(iou, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd, K, iou_thrs, area_rng, max_det, rank, bits,
               npig, seen, dbg_match=None):
    """evaluateImg for B images (include/scda_ops.h: scda_coco_match_hip).  iou float64 [B, G, D]; dt_cat int32 / score float32 / dt_area
    float64 [B, D]; gt_cat int32 / gt_area float64 / gt_iscrowd uint8 [B, G]; iou_thrs float64 [T], area_rng float64 [A, 2] on the device
    -> rank int32 [B, D], bits int32 [B, D, A], and npig int32 [K, A], seen int32 [K] accumulated.  dbg_match int32 [B, D, A, T] or None."""
    _coco_match(False, iou, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd, None, K, iou_thrs, area_rng, max_det,
                rank, bits, npig, seen, dbg_match)


def coco_match_ign(iou, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd, gt_ignore, K, iou_thrs, area_rng,
                   max_det, rank, bits, npig, seen, dbg_match=None):
    """coco_match with the GTs' ignore flags given apart from iscrowd (include/scda_ops.h: scda_coco_match_ign_hip): gt_ignore uint8
    [B, G], or None for iscrowd -- then the results are coco_match's byte for byte"""
    _coco_match(True, iou, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd, gt_ignore, K, iou_thrs, area_rng,
                max_det, rank, bits, npig, seen, dbg_match)


def _coco_match(ign, iou, dt_counts, dt_cat, score, dt_area, gt_counts, gt_cat, gt_area, gt_iscrowd, gt_ignore, K, iou_thrs, area_rng,
                max_det, rank, bits, npig, seen, dbg_match):
    B, D = dt_cat.shape
    G = gt_cat.shape[1]
    T, A = iou_thrs.numel(), area_rng.shape[0]
    _req_all("coco_match", ((iou, "iou", torch.float64, B * G * D), (dt_counts, "dt_counts", torch.int32, B),
                            (dt_cat, "dt_cat", torch.int32, B * D), (score, "score", torch.float32, B * D),
                            (dt_area, "dt_area", torch.float64, B * D), (gt_counts, "gt_counts", torch.int32, B),
                            (gt_cat, "gt_cat", torch.int32, B * G), (gt_area, "gt_area", torch.float64, B * G),
                            (gt_iscrowd, "gt_iscrowd", torch.uint8, B * G), (iou_thrs, "iou_thrs", torch.float64, T),
                            (area_rng, "area_rng", torch.float64, 2 * A), (rank, "rank", torch.int32, B * D),
                            (bits, "bits", torch.int32, B * D * A), (npig, "npig", torch.int32, K * A), (seen, "seen", torch.int32, K))
             + (((dbg_match, "dbg_match", torch.int32, B * D * A * T),) if dbg_match is not None else ())
             + (((gt_ignore, "gt_ignore", torch.uint8, B * G),) if gt_ignore is not None else ()))
    if ign:
        _check(lib().scda_coco_match_ign_hip(_p(iou), B, D, G, _p(dt_counts), _p(dt_cat), _p(score), _p(dt_area), _p(gt_counts),
                                             _p(gt_cat), _p(gt_area), _p(gt_iscrowd), _p(gt_ignore), int(K), _p(iou_thrs), T,
                                             _p(area_rng), A, int(max_det), _p(rank), _p(bits), _p(npig), _p(seen), _p(dbg_match),
                                             _stream()), "scda_coco_match_ign_hip")
        return
    _check(lib().scda_coco_match_hip(_p(iou), B, D, G, _p(dt_counts), _p(dt_cat), _p(score), _p(dt_area), _p(gt_counts), _p(gt_cat),
                                     _p(gt_area), _p(gt_iscrowd), int(K), _p(iou_thrs), T, _p(area_rng), A, int(max_det), _p(rank),
                                     _p(bits), _p(npig), _p(seen), _p(dbg_match), _stream()), "scda_coco_match_hip")


def coco_accumulate_workspace_bytes(n_images, D, K, A):
    return int(lib().scda_coco_accumulate_workspace_bytes(n_images, D, K, A))


def coco_accumulate(image_ids, n_images, cat, rank, score, bits, npig, seen, rec_thrs, max_dets, max_det_last, T, ws, precision, recall,
                    scores):
    """accumulate over the first n_images images' rows (include/scda_ops.h: scda_coco_accumulate_hip); every tensor is the caller's"""
    D = cat.shape[1]
    K, A = npig.shape
    R, M = rec_thrs.numel(), max_dets.numel()
    _req_all("coco_accumulate", ((image_ids, "image_ids", torch.int32, n_images), (cat, "cat", torch.int32, n_images * D),
                                 (rank, "rank", torch.int32, n_images * D), (score, "score", torch.float32, n_images * D),
                                 (bits, "bits", torch.int32, n_images * D * A), (npig, "npig", torch.int32, K * A),
                                 (seen, "seen", torch.int32, K), (rec_thrs, "rec_thrs", torch.float64, R),
                                 (max_dets, "max_dets", torch.int32, M), (precision, "precision", torch.float64, T * R * K * A * M),
                                 (recall, "recall", torch.float64, T * K * A * M), (scores, "scores", torch.float64, T * R * K * A * M),
                                 (ws, "ws", torch.uint8, 1)))
    need = coco_accumulate_workspace_bytes(n_images, D, K, A)
    if need == 0 or ws.numel() < need:
        raise ValueError("coco_accumulate: workspace too small or sizes out of range")
    _check(lib().scda_coco_accumulate_hip(_p(image_ids), n_images, D, _p(cat), _p(rank), _p(score), _p(bits), _p(npig), _p(seen), K, T, A,
                                          _p(rec_thrs), R, _p(max_dets), M, int(max_det_last), _p(ws), _p(precision), _p(recall),
                                          _p(scores), _stream()), "scda_coco_accumulate_hip")


def coco_summarize(precision, recall, shape, spec, stats):
    """_summarizeDets on the device: shape = (T, R, K, A, M), spec int32 [n, 4] = (ap, t, a, m) -> stats float64 [n]"""
    _req(precision, "precision", torch.float64); _req(recall, "recall", torch.float64)
    _req(spec, "spec", torch.int32); _req(stats, "stats", torch.float64)
    T, R, K, A, M = (int(v) for v in shape)
    n = spec.shape[0]
    if precision.numel() != T * R * K * A * M or recall.numel() != T * K * A * M or spec.numel() != 4 * n or stats.numel() < n:
        raise ValueError("coco_summarize: precision [T, R, K, A, M], recall [T, K, A, M], spec [n, 4], stats [n]")
    _check(lib().scda_coco_summarize_hip(_p(precision), _p(recall), T, R, K, A, M, _p(spec), n, _p(stats), _stream()),
           "scda_coco_summarize_hip")
    return stats


# ------------------------------------------------- Cityscapes mAP (cal_mAP) --
def map_rows(detections, detection_counts, image_info, scale_column, num_classes, keep_num, box, score, cls, rank, kept, tp,
             dbg_match=None, dbg_claimed=None, G=1):
    """validate()'s rows of B images (include/scda_ops.h: scda_map_rows_hip, rule R1).  detections float32 [B, D, 7], detection_counts
    int32 [B], image_info float32 [B, >= 2] -> the caller's box int32 [B, D, 4], score float32, cls / rank / kept / tp int32 [B, D];
    dbg_match int32 [B, D] and dbg_claimed int32 [B, G] are reset when given."""
    _req(detections, "detections"); _req(image_info, "image_info")
    if detections.dim() != 3 or detections.shape[2] != 7 or image_info.dim() != 2 or image_info.shape[0] != detections.shape[0]:
        raise ValueError("map_rows: detections [B, D, 7] and image_info [B, >= 2]")
    B, D = detections.shape[:2]
    info_w = image_info.shape[1]
    scale_column = scale_column % info_w if -info_w <= scale_column < info_w else -1
    _req_all("map_rows", ((detection_counts, "detection_counts", torch.int32, B), (box, "box", torch.int32, B * D * 4),
                          (score, "score", torch.float32, B * D), (cls, "cls", torch.int32, B * D), (rank, "rank", torch.int32, B * D),
                          (kept, "kept", torch.int32, B * D), (tp, "tp", torch.int32, B * D))
             + (((dbg_match, "dbg_match", torch.int32, B * D),) if dbg_match is not None else ())
             + (((dbg_claimed, "dbg_claimed", torch.int32, B * G),) if dbg_claimed is not None else ()))
    _check(lib().scda_map_rows_hip(_p(detections), _p(detection_counts), B, D, _p(image_info), info_w, scale_column, int(num_classes),
                                   int(keep_num), _p(box), _p(score), _p(cls), _p(rank), _p(kept), _p(tp), _p(dbg_match), int(G),
                                   _p(dbg_claimed), _stream()), "scda_map_rows_hip")


def map_match(box, cls, rank, kept, gt_boxes, gt_counts, num_classes, iou_thr, tp, gt_num, dbg_match=None, dbg_claimed=None):
    """calIoU and cal_mAP's claims for B images (include/scda_ops.h: scda_map_match_hip, rule R2).  box int32 [B, D, 4], cls / rank /
    kept int32 [B, D] as map_rows wrote them, gt_boxes int32 [B, G, 5] = (x1, y1, x2, y2, label), gt_counts int32 [B] -> tp int32
    [B, D]; gt_num int32 [C] accumulated.  dbg_match int32 [B, D], dbg_claimed int32 [B, G] or None."""
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 5 or cls.dim() != 2 or gt_boxes.shape[0] != cls.shape[0]:
        raise ValueError("map_match: gt_boxes [B, G, 5] and cls [B, D]")
    B, D = cls.shape
    G = gt_boxes.shape[1]
    _req_all("map_match", ((box, "box", torch.int32, B * D * 4), (cls, "cls", torch.int32, B * D), (rank, "rank", torch.int32, B * D),
                           (kept, "kept", torch.int32, B * D), (gt_boxes, "gt_boxes", torch.int32, B * G * 5),
                           (gt_counts, "gt_counts", torch.int32, B), (tp, "tp", torch.int32, B * D),
                           (gt_num, "gt_num", torch.int32, int(num_classes)))
             + (((dbg_match, "dbg_match", torch.int32, B * D),) if dbg_match is not None else ())
             + (((dbg_claimed, "dbg_claimed", torch.int32, B * G),) if dbg_claimed is not None else ()))
    _check(lib().scda_map_match_hip(_p(box), _p(cls), _p(rank), _p(kept), B, D, _p(gt_boxes), _p(gt_counts), G, int(num_classes),
                                    float(iou_thr), _p(tp), _p(gt_num), _p(dbg_match), _p(dbg_claimed), _stream()), "scda_map_match_hip")


def map_recall(proposals, proposal_counts, gts, gt_counts, counters):
    """compute_recall for B images (include/scda_ops.h: scda_map_recall_hip, rule R4).  proposals float32 [B, P, >= 5] (columns 1..4),
    proposal_counts int32 [B], gts float32 [B, Gr, >= 4], gt_counts int32 [B] -> counters int32 [2] += (recalled, rows given)."""
    _req(proposals, "proposals"); _req(gts, "gts")
    if proposals.dim() != 3 or gts.dim() != 3 or gts.shape[0] != proposals.shape[0]:
        raise ValueError("map_recall: proposals [B, P, >= 5] and gts [B, Gr, >= 4]")
    B = proposals.shape[0]
    _req_all("map_recall", ((proposal_counts, "proposal_counts", torch.int32, B), (gt_counts, "gt_counts", torch.int32, B),
                            (counters, "counters", torch.int32, 2)))
    _check(lib().scda_map_recall_hip(_p(proposals), _p(proposal_counts), B, proposals.shape[1], proposals.shape[2], _p(gts),
                                     _p(gt_counts), gts.shape[1], gts.shape[2], _p(counters), _stream()), "scda_map_recall_hip")


def map_accumulate_workspace_bytes(n_images, D):
    return int(lib().scda_map_accumulate_workspace_bytes(n_images, D))


def map_accumulate(n_images, score, cls, rank, kept, tp, sum_gt, ws, ap, max_recall, rows):
    """cal_mAP's accumulation over the first n_images images' rows (include/scda_ops.h: scda_map_accumulate_hip, rule R3); sum_gt int32
    [C] on the device -> ap, max_recall float64 [C], rows int32 [C]; every tensor is the caller's"""
    D, C = cls.shape[1], sum_gt.numel()
    _req_all("map_accumulate", ((score, "score", torch.float32, n_images * D), (cls, "cls", torch.int32, n_images * D),
                                (rank, "rank", torch.int32, n_images * D), (kept, "kept", torch.int32, n_images * D),
                                (tp, "tp", torch.int32, n_images * D), (sum_gt, "sum_gt", torch.int32, C), (ap, "ap", torch.float64, C),
                                (max_recall, "max_recall", torch.float64, C), (rows, "rows", torch.int32, C), (ws, "ws", torch.uint8, 1)))
    need = map_accumulate_workspace_bytes(n_images, D)
    if need == 0 or ws.numel() < need:
        raise ValueError("map_accumulate: workspace too small or sizes out of range")
    _check(lib().scda_map_accumulate_hip(n_images, D, _p(score), _p(cls), _p(rank), _p(kept), _p(tp), _p(sum_gt), C, _p(ws), _p(ap),
                                         _p(max_recall), _p(rows), _stream()), "scda_map_accumulate_hip")


# ------------------------------------------------- merging sharded evaluators --
EVAL_FILL = {"zero": 0, "slot": 1, "minus_one": 2}
MAX_SHARDS = 256


def eval_place_rows(src, order, counts, start, dst, flags, fill="zero"):
    """One row array of W gathered shards into an evaluator's rows (include/scda_ops.h: scda_eval_place_rows_hip, rule M1).  src
    [W, cap, ...] and dst [max_images, ...] of one 4- or 8-byte dtype and one row shape; order: a permutation of range(W) on the host;
    counts: W host integers, or an int32 [W] device tensor (then every slot from `start` on is written, `fill` behind the total);
    flags int32 [4]."""
    if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()) or src.dtype != dst.dtype or \
            src.element_size() not in (4, 8) or src.dim() < 2 or tuple(src.shape[2:]) != tuple(dst.shape[1:]):
        raise ValueError("eval_place_rows: src [W, cap, ...] and dst [max_images, ...] contiguous device tensors of one 4- or 8-byte dtype")
    _req(flags, "flags", torch.int32)
    W, cap = int(src.shape[0]), int(src.shape[1])
    words = (src[0, 0].numel() if src.dim() > 2 else 1) * src.element_size() // 4
    if W > MAX_SHARDS or len(order) != W or flags.numel() < 4:
        raise ValueError("eval_place_rows: at most %d shards, one order entry per shard, flags [4]" % MAX_SHARDS)
    order_c = (ctypes.c_int * W)(*[int(o) for o in order])
    on_device = torch.is_tensor(counts)
    if on_device:
        _req(counts, "counts", torch.int32)
        if counts.numel() != W:
            raise ValueError("eval_place_rows: counts must hold one entry per shard")
    else:
        counts_c = (ctypes.c_int * W)(*[int(c) for c in counts])
    _check(lib().scda_eval_place_rows_hip(_p(src), W, cap, words, order_c, None if on_device else counts_c, _p(counts) if on_device else None,
                                          int(start), int(dst.shape[0]), EVAL_FILL[fill], _p(dst), _p(flags), _stream()),
           "scda_eval_place_rows_hip")


def eval_sum_counters(src, dst):
    """dst int32 [n] += the sum over the shards of src int32 [W, n] (scda_eval_sum_counters_hip, rule M2)"""
    W = int(src.shape[0])
    n = dst.numel()
    _req_all("eval_sum_counters", ((src, "src", torch.int32, W * n), (dst, "dst", torch.int32, n)))
    if src.numel() != W * n:
        raise ValueError("eval_sum_counters: src must be [W, %d]" % n)
    _check(lib().scda_eval_sum_counters_hip(_p(src), W, n, _p(dst), _stream()), "scda_eval_sum_counters_hip")


def eval_mark_duplicates_workspace_bytes(n):
    return int(lib().scda_eval_mark_duplicates_workspace_bytes(n))


def eval_mark_duplicates(image_ids, n, ws, first, flags, raise_on_duplicate=False):
    """first int32 [n] = the first merged position of a repeated image id >= 0, else -1; flags[2] = the number of duplicates
    (scda_eval_mark_duplicates_hip, rule M3)"""
    _req_all("eval_mark_duplicates", ((image_ids, "image_ids", torch.int32, n), (first, "first", torch.int32, n),
                                      (flags, "flags", torch.int32, 4), (ws, "ws", torch.uint8, 1)))
    need = eval_mark_duplicates_workspace_bytes(n)
    if need == 0 or ws.numel() < need:
        raise ValueError("eval_mark_duplicates: workspace too small or n out of range")
    _check(lib().scda_eval_mark_duplicates_hip(_p(image_ids), int(n), _p(ws), _p(first), _p(flags), 1 if raise_on_duplicate else 0,
                                               _stream()), "scda_eval_mark_duplicates_hip")


def map_merge_duplicates(first, n, box, score, cls, rank, kept, tp, flags):
    """cal_mAP's treatment of a repeated image: tp = 0 for the rows of every later copy; flags[1] = 1 if a copy's rows differ from the
    first copy's (scda_map_merge_duplicates_hip, rule M4)"""
    D = cls.shape[1]
    _req_all("map_merge_duplicates", ((first, "first", torch.int32, n), (box, "box", torch.int32, n * D * 4),
                                      (score, "score", torch.float32, n * D), (cls, "cls", torch.int32, n * D),
                                      (rank, "rank", torch.int32, n * D), (kept, "kept", torch.int32, n * D), (tp, "tp", torch.int32, n * D),
                                      (flags, "flags", torch.int32, 4)))
    _check(lib().scda_map_merge_duplicates_hip(_p(first), int(n), D, _p(box), _p(score), _p(cls), _p(rank), _p(kept), _p(tp), _p(flags),
                                               _stream()), "scda_map_merge_duplicates_hip")


# ------------------------------------------------- convolution / GEMM -------
_WS = {}


def workspace(nbytes, device):
    """Grow-only scratch buffer (split-K slabs), one per (device, stream): kernels on different HIP streams may run
    concurrently and must not share slabs.  Never freed during a run."""
    key = (device.index, _stream())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def _conv_ws(batch, cin, ih, iw, cout, kh, kw, s, p, device):
    L = lib()
    n = L.scda_conv2d_workspace_bytes(batch, cin, ih, iw, cout, kh, kw, s, p)
    return workspace(n, device), n


WEIGHT_EPOCH = [0]   # fallback epoch for weights that are not part of a FlatParams bucket (bump after raw-pointer updates)
_PACK_CACHE = {}


def _pack_tag(w):
    """what a packed copy of `w` was made from: the pack cache serves an entry only under an equal tag.  A weight inside a FlatParams
    bucket is written three ways, and each moves one field: a torch op on the Parameter bumps w._version; a torch op on the bucket
    (flat.data, FlatAdam's bucket Parameter, any detached alias or slice of them: they share ONE counter, which `p.data = view` does
    NOT hand to the Parameter) bumps flat.data._version; a kernel or collective that writes through raw pointers bumps neither, so
    whoever launches it bumps flat.epoch (FlatAdam.step, checkpoint.restore, broadcast_params) -- or WEIGHT_EPOCH for a weight
    outside every bucket."""
    flat = getattr(w, "_scda_flat", None)
    if flat is None:
        return (w._version, WEIGHT_EPOCH[0], 0, tuple(w.shape))
    return (w._version, flat.epoch, flat.data._version, tuple(w.shape))


def conv2d_pack_weight(w, for_dgrad=False, cache=True):
    """[Cout,Cin,KH,KW] -> the library's GEMM-ready layout for the forward / data-gradient kernel (see scda_ops.h).
    Cached per (storage, direction) until the weight changes (tensor version or optimiser epoch)."""
    _req(w, "w")
    Cout, Cin, KH, KW = w.shape
    # only parameters are worth caching: a temporary (e.g. the transposed 1x1 weight of ConvTranspose1x1) gets a new address
    # on every call and would leave a dead entry behind each time
    cache = cache and isinstance(w, torch.nn.Parameter)
    key = (w.data_ptr(), for_dgrad)
    tag = _pack_tag(w)
    if cache:
        hit = _PACK_CACHE.get(key)
        # valid only for the very same tensor object (a freed temporary's address may be reused by another weight)
        if hit is not None and hit[0] == tag and hit[2]() is w:
            return hit[1]
    n = lib().scda_conv2d_packed_elems(Cout, Cin, KH, KW, int(for_dgrad))
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    _check(lib().scda_conv2d_pack_weight_hip(_p(w), _p(out), Cout, Cin, KH, KW, int(for_dgrad), _stream()), "scda_conv2d_pack_weight_hip")
    if cache:
        _PACK_CACHE[key] = (tag, out, weakref.ref(w))
    return out


def wino_enabled():
    """the stride-1 3x3 layers the Winograd kernels support run on them (SCDA_WINOGRAD=0: every layer on the direct implicit-GEMM kernels)"""
    return bool(lib().scda_conv2d_wino_enabled())


def _route(direction, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period):
    """csrc/launch_plan.h route_conv: (family 0 implicit GEMM / 1 Winograd / 2 Winograd on stacked 7 x 7 maps, conv + pool fusable, maps)"""
    pool, maps = ctypes.c_int(0), ctypes.c_int(0)
    fam = lib().scda_conv2d_route(direction, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period, ctypes.byref(pool), ctypes.byref(maps))
    return fam, bool(pool.value), maps.value


def wino_stacked(B, IH, IW, row_period):
    """the image is a stack of 7 x 7 maps (the ResNet-50 C4 detector's channel-major RoI head): -> number of maps, else 0"""
    return _route(0, B, 0, IH, IW, 0, 3, 3, 1, 1, row_period)[2]


def wino_ok(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period=0):
    """this convolution (forward: reduced channels Cin, output rows Cout) takes the Winograd path"""
    return _route(0, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)[0] != 0


def wino_wgrad_ok(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period=0):
    """this weight gradient takes the Winograd kernel"""
    return _route(2, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)[0] != 0


def conv2d_wino_wgrad(dy, x, w_shape, out=None, db_out=None, want_bias=False, row_period=0):
    """(dw, db) of a stride-1 pad-1 3x3 convolution on the Winograd weight-gradient kernel; accumulates into out / db_out when given"""
    _req(dy, "dy"); _req(x, "x")
    B, Cin, IH, IW = x.shape
    Cout = w_shape[0]
    acc = dbacc = 0
    if out is None:
        out = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    else:
        _req(out, "out"); acc = 1
    db = None
    if want_bias or db_out is not None:
        if db_out is None:
            db = torch.empty(Cout, dtype=torch.float32, device=x.device)
        else:
            _req(db_out, "db_out"); db = db_out; dbacc = 1
    ws, n = _conv_ws(B, Cin, IH, IW, Cout, 3, 3, 1, 1, x.device)
    if row_period:
        maps = wino_stacked(B, IH, IW, row_period)
        if not maps:
            raise ValueError("conv2d_wino_wgrad: row_period %d on %s is not a stack of 7 x 7 maps" % (row_period, tuple(x.shape)))
        _check(lib().scda_conv2d_wino_wgrad_stacked_hip(_p(dy), _p(x), _p(out), _p(db), maps, Cin, Cout, acc, dbacc, _p(ws), n, _stream()),
               "scda_conv2d_wino_wgrad_stacked_hip")
        return out, db
    _check(lib().scda_conv2d_wino_wgrad_hip(_p(dy), _p(x), _p(out), _p(db), B, Cin, IH, IW, Cout, acc, dbacc, _p(ws), n, _stream()),
           "scda_conv2d_wino_wgrad_hip")
    return out, db


def conv2d_wino_pack(w, for_dgrad=False, cache=True):
    """[Cout,Cin,3,3] -> the Winograd kernel's transformed filters (scda_ops.h), cached like conv2d_pack_weight's layouts"""
    _req(w, "w")
    Cout, Cin, KH, KW = w.shape
    cache = cache and isinstance(w, torch.nn.Parameter)
    key = (w.data_ptr(), 2 + int(for_dgrad))
    tag = _pack_tag(w)
    if cache:
        hit = _PACK_CACHE.get(key)
        if hit is not None and hit[0] == tag and hit[2]() is w:
            return hit[1]
    L = lib()
    n = L.scda_conv2d_wino_packed_elems(Cout, Cin, int(for_dgrad))
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    _check(L.scda_conv2d_wino_pack_hip(_p(w.contiguous()), _p(out), Cout, Cin, int(for_dgrad), _stream()), "scda_conv2d_wino_pack_hip")
    if cache:
        _PACK_CACHE[key] = (tag, out, weakref.ref(w))
    return out


def _req_wino(x, u, bias, M, mask_src=None):
    """the Winograd launches read the bias dword by dword from its first element (x and the mask are checked by the callers, the packed
    filters come from conv2d_wino_pack): a strided or short one is refused here"""
    if bias is not None and (not bias.is_contiguous() or bias.numel() != M or bias.dtype != torch.float32):
        raise ValueError(f"conv2d_wino: bias must be {M} contiguous float32 values, got {tuple(bias.shape)} {bias.dtype}")


def conv2d_wino(x, u, bias, M, act=ACT_NONE, slope=0.01, mask_src=None, mask_slope=0.0, for_dgrad=False, row_period=0):
    """one Winograd launch: y [B, M, H, W] from x [B, C, H, W] and packed filters u (forward, or the data gradient with x = dy);
    row_period = 7 on a [1, C, R * 7, 7] tensor: a stack of R independent 7 x 7 maps"""
    _req_wino(x, u, bias, M, mask_src)
    B, C, H, W = x.shape
    y = torch.empty(B, M, H, W, dtype=torch.float32, device=x.device)
    ws, n = _conv_ws(B, C, H, W, M, 3, 3, 1, 1, x.device)
    if row_period:
        maps = wino_stacked(B, H, W, row_period)
        if not maps:
            raise ValueError("conv2d_wino: row_period %d on %s is not a stack of 7 x 7 maps" % (row_period, tuple(x.shape)))
        _check(lib().scda_conv2d_wino_stacked_hip(_p(x), _p(u), _p(bias), _p(y), maps, C, M, act, slope, _p(mask_src), mask_slope,
                                                  int(for_dgrad), _p(ws), n, _stream()), "scda_conv2d_wino_stacked_hip")
        return y
    _check(lib().scda_conv2d_wino_hip(_p(x), _p(u), _p(bias), _p(y), B, C, H, W, M, act, slope, _p(mask_src), mask_slope, int(for_dgrad),
                                      _p(ws), n, _stream()), "scda_conv2d_wino_hip")
    return y


def conv_pool_fusable(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period=0):
    """conv3x3 + activation + 2x2 max-pool can run as one Winograd launch: an eligible layer on an even map with enough tiles to fill the
    chip without split-K (the fused epilogue needs finished values).  SCDA_CONV_POOL_FUSE=0 keeps the pool a launch of its own."""
    return _route(0, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)[1]


def conv2d_wino_pool(x, u, bias, M, act=ACT_NONE, slope=0.01):
    """-> (pooled [B, M, H/2, W/2], winner uint8 [B, M, H/2, W/2]) of maxpool2x2(act(conv3x3(x) + bias)), one launch"""
    _req_wino(x, u, bias, M)
    B, C, H, W = x.shape
    y = torch.empty(B, M, H // 2, W // 2, dtype=torch.float32, device=x.device)
    idx = torch.empty(B, M, H // 2, W // 2, dtype=torch.uint8, device=x.device)
    _check(lib().scda_conv2d_wino_pool_hip(_p(x), _p(u), _p(bias), _p(y), _p(idx), B, C, H, W, M, act, slope, _stream()),
           "scda_conv2d_wino_pool_hip")
    return y, idx


def conv2d_pack_all(flat):
    """Re-pack every conv weight of a FlatParams bucket (forward and data-gradient layouts) with ONE launch and seed the
    pack cache with the results.  Called by FlatAdam.step(): the lazy per-layer path above then never misses in the
    training loop (it was 90 five-microsecond launches per iteration, each a dependent dispatch on the compute stream)."""
    ws = getattr(flat, "conv_weights", None)
    if not ws:
        return
    # which weights ran on the Winograd kernel in their last forward call (native.conv2d_fwd notes it): those get its transformed
    # filters (modes 2, 3) instead of the implicit-GEMM layouts (0, 1); a call that needs the other kind packs lazily
    wino = tuple(bool(getattr(w, "_scda_wino_used", False)) for w in ws) if wino_enabled() else None
    # one plan (descriptor table + output buffer) PER flag tuple, kept: with variable-size inputs a layer's eligibility flips with the
    # parity of the map size, and rebuilding the plan on every flip meant a descriptor upload and fresh buffers for every layout
    plans = flat.__dict__.setdefault("_scda_pack_plans", {})
    plan = plans.get(wino)
    L = lib()
    if plan is None:
        rows, entries, off, tiles = [], [], 0, 0
        base = flat.data.data_ptr()
        for i, w in enumerate(ws):
            Cout, Cin, KH, KW = w.shape
            src = (w.data_ptr() - base) // 4
            use_wino = wino is not None and wino[i] and all(L.scda_conv2d_packed_elems(Cout, Cin, KH, KW, d) for d in (2, 3))
            for d in ((2, 3) if use_wino else (0, 1)):
                n = int(L.scda_conv2d_packed_elems(Cout, Cin, KH, KW, d))
                rows.append([src, off, Cout, Cin, KH * KW, d, tiles])
                entries.append((w, d if d >= 2 else bool(d), off, n))
                off += n
                tiles += int(L.scda_conv2d_pack_tiles(Cout, Cin, KH, KW, d))
        desc = upload(torch.tensor(rows, dtype=torch.int64), flat.data.device)
        while len(plans) >= 4:       # least recently used first (dicts keep insertion order; a hit re-inserts below)
            plans.pop(next(iter(plans)))
        plan = (desc, off, entries, tiles, wino)
    else:
        plans.pop(wino)
    plans[wino] = plan
    desc, total, entries, tiles, _ = plan
    # ONE output buffer for every plan, sized for the largest layout: a plan is a descriptor table, not a copy of the packed weights
    # (eight kept plans were eight such buffers -- several hundred MB for VGG16 with variable-size inputs).  Sharing is safe: this
    # function runs behind an optimiser step, whose epoch bump has already invalidated every cache entry of the previous layout.
    out = flat.__dict__.get("_scda_pack_out")
    if out is None or out.numel() < total:
        out = flat.__dict__["_scda_pack_out"] = torch.empty(total, dtype=torch.float32, device=flat.data.device)
    _check(L.scda_conv2d_pack_weights_batched_hip(_p(flat.data), _p(out), _p(desc), len(entries), tiles, _stream()),
           "scda_conv2d_pack_weights_batched_hip")
    for w, d, off, n in entries:
        if w.data_ptr() < flat.data.data_ptr():   # parameter was re-homed: fall back to the lazy path for it
            continue
        _PACK_CACHE[(w.data_ptr(), d)] = (_pack_tag(w), out[off:off + n], weakref.ref(w))


def conv2d_fwd(x, w, bias, stride, pad, act=ACT_NONE, slope=0.01, row_period=0):
    _req(x, "x"); _req(w, "w")
    if bias is not None:
        _req(bias, "bias")
    B, Cin, IH, IW = x.shape
    Cout, Cin2, KH, KW = w.shape
    if Cin2 != Cin:
        raise ValueError(f"conv2d: input has {Cin} channels, weight expects {Cin2}")
    OH = (IH + 2 * pad - KH) // stride + 1
    OW = (IW + 2 * pad - KW) // stride + 1
    use_wino = wino_ok(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)
    if isinstance(w, torch.nn.Parameter):
        w._scda_wino_used = use_wino       # conv2d_pack_all re-packs the layouts the layer's calls actually use
    if use_wino:
        return conv2d_wino(x, conv2d_wino_pack(w, False), bias, Cout, act, slope, row_period=row_period)
    wp = conv2d_pack_weight(w, False)
    y = torch.empty(B, Cout, OH, OW, dtype=torch.float32, device=x.device)
    ws, n = _conv_ws(B, Cin, IH, IW, Cout, KH, KW, stride, pad, x.device)
    _check(lib().scda_conv2d_fwd_hip(_p(x), _p(wp), _p(bias), _p(y), B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period, act, slope,
                                     _p(ws), n, _stream()), "scda_conv2d_fwd_hip")
    return y


def conv2d_dgrad(dy, w, x_shape, stride, pad, act_src=None, act_slope=0.0, row_period=0):
    """act_src (the conv's input x, a ReLU / LeakyReLU output): dx is additionally multiplied by x > 0 ? 1 : act_slope -- the
    activation gradient of the layer that produced x, folded into this kernel's epilogue"""
    _req(dy, "dy"); _req(w, "w")
    B, Cin, IH, IW = x_shape
    Cout, _, KH, KW = w.shape
    if act_src is not None:
        _req(act_src, "act_src")
        if tuple(act_src.shape) != tuple(x_shape):
            raise ValueError("act_src must have the shape of the conv input")
    if _route(1, B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)[0]:
        return conv2d_wino(dy, conv2d_wino_pack(w, True), None, Cin, ACT_NONE, 0.0, act_src, act_slope, for_dgrad=True, row_period=row_period)
    dx = torch.empty(B, Cin, IH, IW, dtype=torch.float32, device=dy.device)
    if act_src is None and Cin <= 4 and Cout * KH * KW * 16 <= 65536 and (KH, KW) in ((3, 3), (1, 1)):
        # image-side layer: 3 rows of a 64-row MFMA tile would be 95 % padding -- direct kernel, unpacked weights
        _check(lib().scda_conv2d_dgrad_small_cin_hip(_p(dy), _p(w.contiguous()), _p(dx), B, Cin, IH, IW, Cout, KH, KW, stride, pad,
                                                     _stream()), "scda_conv2d_dgrad_small_cin_hip")
        return dx
    wt = conv2d_pack_weight(w, True)
    ws, n = _conv_ws(B, Cin, IH, IW, Cout, KH, KW, stride, pad, dy.device)
    _check(lib().scda_conv2d_dgrad_act_hip(_p(dy), _p(wt), _p(dx), B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period, _p(act_src),
                                           act_slope, _p(ws), n, _stream()), "scda_conv2d_dgrad_act_hip")
    return dx


def conv2d_wgrad(dy, x, w_shape, stride, pad, out=None, row_period=0):
    """dw = wgrad(dy, x); with `out` given, accumulates into it."""
    _req(dy, "dy"); _req(x, "x")
    B, Cin, IH, IW = x.shape
    Cout, _, KH, KW = w_shape
    if wino_wgrad_ok(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period):
        return conv2d_wino_wgrad(dy, x, w_shape, out=out, row_period=row_period)[0]
    acc = 0
    if out is None:
        out = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    else:
        _req(out, "out"); acc = 1
    ws, n = _conv_ws(B, Cin, IH, IW, Cout, KH, KW, stride, pad, x.device)
    _check(lib().scda_conv2d_wgrad_hip(_p(dy), _p(x), _p(out), B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period, acc, _p(ws), n,
                                       _stream()), "scda_conv2d_wgrad_hip")
    return out


def conv2d_wgrad_bias(dy, x, w_shape, stride, pad, out=None, db_out=None, row_period=0):
    """(dw, db): weight and bias gradient of a conv layer.  One fused pass (the bias gradient rides on the weight-gradient
    GEMM's operand fragments) when the library says the shape allows it, otherwise the two separate kernels.  `out` /
    `db_out` given: accumulate into them."""
    _req(dy, "dy"); _req(x, "x")
    B, Cin, IH, IW = x.shape
    Cout, _, KH, KW = w_shape
    if wino_wgrad_ok(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period):
        return conv2d_wino_wgrad(dy, x, w_shape, out=out, db_out=db_out, want_bias=True, row_period=row_period)
    L = lib()
    if not L.scda_conv2d_wgrad_bias_fusable(B, Cout, dy.shape[2], dy.shape[3], _p(dy)):
        return conv2d_wgrad(dy, x, w_shape, stride, pad, out=out, row_period=row_period), bias_grad_nchw(dy, out=db_out)
    acc = dbacc = 0
    if out is None:
        out = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    else:
        _req(out, "out"); acc = 1
    if db_out is None:
        db_out = torch.empty(Cout, dtype=torch.float32, device=x.device)
    else:
        _req(db_out, "db_out"); dbacc = 1
    ws, n = _conv_ws(B, Cin, IH, IW, Cout, KH, KW, stride, pad, x.device)
    _check(L.scda_conv2d_wgrad_bias_hip(_p(dy), _p(x), _p(out), _p(db_out), B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period, acc,
                                        dbacc, _p(ws), n, _stream()), "scda_conv2d_wgrad_bias_hip")
    return out, db_out


def conv2d_bias_grad(dy, x, w_shape, stride, pad, out=None, row_period=0):
    """db of a conv layer on its own, with the bits conv2d_wgrad_bias gives for the layer: where that call runs a kernel with the
    bias gradient fused in (Winograd, or the fusable direct shapes) the same kernel runs here and its weight gradient is dropped, so
    a gradient does not depend on which others were asked for.  (No SCDA net trains a bias under a frozen weight.)"""
    _req(dy, "dy"); _req(x, "x")
    B, Cin, IH, IW = x.shape
    Cout, _, KH, KW = w_shape
    if not (wino_wgrad_ok(B, Cin, IH, IW, Cout, KH, KW, stride, pad, row_period)
            or lib().scda_conv2d_wgrad_bias_fusable(B, Cout, dy.shape[2], dy.shape[3], _p(dy))):
        return bias_grad_nchw(dy, out=out)
    return conv2d_wgrad_bias(dy, x, w_shape, stride, pad, db_out=out, row_period=row_period)[1]


def gemm(a, b, M, N, K, lda, ldb, trans_a=False, trans_b=False, bias=None, bias_on_n=True, act=ACT_NONE, slope=0.01,
         out=None, accumulate=False):
    """C[M,N] (+)= op(A) op(B) (+bias) -> act.  See include/scda_ops.h for the operand layouts."""
    _req(a, "a"); _req(b, "b")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    else:
        _req(out, "out")
    L = lib()
    n = L.scda_gemm_workspace_bytes(M, N, K)
    ws = workspace(n, a.device)
    _check(L.scda_gemm_hip(_p(a), _p(b), _p(out), M, N, K, lda, ldb, N, int(trans_a), int(trans_b), _p(bias), int(bias_on_n), act, slope,
                           int(accumulate), _p(ws), n, _stream()), "scda_gemm_hip")
    return out


def linear_fwd(x, w, bias, act=ACT_NONE):
    """y[M,out] = x[M,in] @ w[out,in]^T + b"""
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:          # (gemm checks device, dtype and contiguity)
        raise ValueError(f"linear: x {tuple(x.shape)} and w {tuple(w.shape)} must be [M,in] and [out,in]")
    M, K = x.shape
    N = w.shape[0]
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != N:
            raise ValueError(f"linear: bias must have {N} values, got {bias.numel()}")
    return gemm(x, w, M, N, K, K, K, False, False, bias, True, act)


def linear_dgrad(dy, w):
    """dx[M,in] = dy[M,out] @ w[out,in]"""
    if dy.dim() != 2 or w.dim() != 2 or w.shape[0] != dy.shape[1]:
        raise ValueError(f"linear: dy {tuple(dy.shape)} and w {tuple(w.shape)} must be [M,out] and [out,in]")
    M, K = dy.shape
    N = w.shape[1]
    return gemm(dy, w, M, N, K, K, N, False, True)


def linear_wgrad(dy, x, out=None, accumulate=True):
    """dw[out,in] (+)= dy[M,out]^T @ x[M,in]; with `out`: accumulates into it unless accumulate=False (overwrite)"""
    if dy.dim() != 2 or x.dim() != 2 or x.shape[0] != dy.shape[0]:
        raise ValueError(f"linear: dy {tuple(dy.shape)} and x {tuple(x.shape)} must be [M,out] and [M,in]")
    Kb, M = dy.shape
    N = x.shape[1]
    if out is not None and out.numel() != M * N:
        raise ValueError(f"linear: the weight gradient has {M * N} values, out {out.numel()}")
    return gemm(dy, x, M, N, Kb, M, N, True, True, out=out, accumulate=out is not None and accumulate)


# ------------------------------------------------------ layer kernels -------
def _req_like(t, name, ref, ref_name, dtype=torch.float32):
    """t: a contiguous device tensor of `dtype` with as many elements as `ref`"""
    if _req(t, name, dtype).numel() != ref.numel():
        raise ValueError(f"{name} must have the {ref.numel()} elements of {ref_name}, got {t.numel()}")
    return t


def _req_channels(C, **vectors):
    """per-channel vectors of a batch norm (None: not given): contiguous float32 of C elements each"""
    for name, v in vectors.items():
        if v is not None and _req(v, name).numel() != C:
            raise ValueError(f"{name} must have one value per channel ({C}), got {v.numel()}")


def _req_map(x, name="x"):
    if _req(x, name).dim() != 4:
        raise ValueError(f"{name} must be [B, C, H, W], got {tuple(x.shape)}")
    return x.shape


def maxpool2x2_fwd(x):
    _req(x, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    idx = torch.empty(B, C, H // 2, W // 2, dtype=torch.uint8, device=x.device)
    _check(lib().scda_maxpool2x2_fwd_hip(_p(x), _p(y), _p(idx), B * C, H, W, _stream()), "scda_maxpool2x2_fwd_hip")
    return y, idx


def maxpool2x2_bwd(dy, idx, x_shape, relu_y=None):
    """relu_y = the pool's output: additionally applies the gradient of a ReLU that produced the pool's input"""
    _req(dy, "dy"); _req(idx, "idx", torch.uint8)
    B, C, H, W = x_shape
    if tuple(dy.shape) != (B, C, H // 2, W // 2) or idx.shape != dy.shape:
        raise ValueError(f"maxpool2x2_bwd: dy and idx must be {(B, C, H // 2, W // 2)}, got {tuple(dy.shape)} and {tuple(idx.shape)}")
    dx = torch.empty(B, C, H, W, dtype=torch.float32, device=dy.device)
    if relu_y is None:
        _check(lib().scda_maxpool2x2_bwd_hip(_p(dy), _p(idx), _p(dx), B * C, H, W, _stream()), "scda_maxpool2x2_bwd_hip")
    else:
        _req_like(relu_y, "relu_y", dy, "dy")
        _check(lib().scda_maxpool2x2_bwd_relu_hip(_p(dy), _p(idx), _p(relu_y), _p(dx), B * C, H, W, _stream()),
               "scda_maxpool2x2_bwd_relu_hip")
    return dx


def maxpool3x3s2_fwd(x):
    _req(x, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, dtype=torch.float32, device=x.device)
    _check(lib().scda_maxpool3x3s2_fwd_hip(_p(x), _p(y), B * C, H, W, _stream()), "scda_maxpool3x3s2_fwd_hip")
    return y


def add_relu(a, b):
    _req(a, "a"); _req(b, "b")
    if a.shape != b.shape:
        raise ValueError("add_relu: shape mismatch")
    y = torch.empty_like(a)
    _check(lib().scda_add_relu_hip(_p(a), _p(b), _p(y), a.numel(), _stream()), "scda_add_relu_hip")
    return y


ACT_MODE = {"relu": 0, "leaky": 1, "tanh": 2, "sigmoid": 3}


def act_fwd(x, mode, slope=0.01):
    _req(x, "x")
    y = torch.empty_like(x)
    _check(lib().scda_act_fwd_hip(_p(x), _p(y), x.numel(), mode, slope, _stream()), "scda_act_fwd_hip")
    return y


def act_bwd(dy, y, mode, slope=0.01):
    _req(dy, "dy"); _req_like(y, "y", dy, "dy")
    dx = torch.empty_like(dy)
    _check(lib().scda_act_bwd_hip(_p(dy), _p(y), _p(dx), dy.numel(), mode, slope, _stream()), "scda_act_bwd_hip")
    return dx


def axpby(a, b, alpha=1.0, beta=1.0):
    _req(a, "a")
    if b is not None:
        _req_like(b, "b", a, "a")
    y = torch.empty_like(a)
    _check(lib().scda_axpby_hip(_p(a), _p(b), _p(y), a.numel(), alpha, beta, _stream()), "scda_axpby_hip")
    return y


def dropout_mask(shape, p, seed, device):
    mask = torch.empty(shape, dtype=torch.uint8, device=device)
    _check(lib().scda_dropout_mask_hip(_p(mask), mask.numel(), p, seed & 0xFFFFFFFFFFFFFFFF, _stream()), "scda_dropout_mask_hip")
    return mask


def dropout_apply(x, mask, scale):
    _req(x, "x"); _req_like(mask, "mask", x, "x", torch.uint8)
    y = torch.empty_like(x)
    _check(lib().scda_dropout_apply_hip(_p(x), _p(mask), _p(y), x.numel(), scale, _stream()), "scda_dropout_apply_hip")
    return y


def dropout_seeded(x, p, seed, scale, relu_src=None):
    """y = keep(seed, i) ? x * scale : 0 (no mask tensor; the backward calls this again with dy); relu_src: see scda_ops.h"""
    _req(x, "x")
    if relu_src is not None:
        _req_like(relu_src, "relu_src", x, "x")
    y = torch.empty_like(x)
    _check(lib().scda_dropout_seeded_hip(_p(x), _p(y), x.numel(), p, seed & 0xFFFFFFFFFFFFFFFF, scale, _p(relu_src), _stream()),
           "scda_dropout_seeded_hip")
    return y


def sigmoid_bce_rows_fwd(x, t, w, scale, out=None, want_prob=True):
    """out[0] (+)= scale * sum_c w[c] * mean_i BCE(sigmoid(x[c,i]), t[c or 0, i]); -> (out [1], prob [C,n] | None)"""
    _req(x, "x"); _req(t, "t")
    if x.dim() != 2:
        raise ValueError("logits must be [C,n]")
    C, n = x.shape
    t_rows = t.numel() // n if n else 0
    if t.numel() != t_rows * n or t_rows not in (1, C):
        raise ValueError("labels must be [1,n] or [C,n]")
    if w is not None:
        _req(w, "w")
        if w.numel() != C:
            raise ValueError(f"weights must have one value per row ({C}), got {w.numel()}")
    if out is not None:
        _req(out, "out")
        if out.numel() != 1:
            raise ValueError("out must hold one value")
    acc = out is not None
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    prob = torch.empty_like(x) if want_prob else None
    _check(lib().scda_sigmoid_bce_rows_fwd_hip(_p(x), _p(t), t_rows, _p(w), C, n, scale, int(acc), _p(prob), _p(out), _stream()),
           "scda_sigmoid_bce_rows_fwd_hip")
    return out, prob


def sigmoid_bce_rows_bwd(prob, t, w, scale, g):
    _req(prob, "prob"); _req(t, "t"); _req(g, "g")
    if prob.dim() != 2:
        raise ValueError("prob must be [C,n]")
    C, n = prob.shape
    t_rows = t.numel() // n if n else 0
    if t.numel() != t_rows * n or t_rows not in (1, C):
        raise ValueError("labels must be [1,n] or [C,n]")
    if w is not None:
        _req(w, "w")
        if w.numel() != C:
            raise ValueError(f"weights must have one value per row ({C}), got {w.numel()}")
    if g.numel() != 1:
        raise ValueError("g must hold one value")
    dx = torch.empty_like(prob)
    _check(lib().scda_sigmoid_bce_rows_bwd_hip(_p(prob), _p(t), t_rows, _p(w), C, n, scale, _p(g), _p(dx), _stream()),
           "scda_sigmoid_bce_rows_bwd_hip")
    return dx


def bias_grad_nchw(dy, out=None):
    """db[c] = sum over batch and pixels; with `out` given, accumulates into it"""
    _req(dy, "dy")
    B, C = dy.shape[0], dy.shape[1]
    HW = dy.numel() // (B * C)
    db = out if out is not None else torch.empty(C, dtype=torch.float32, device=dy.device)
    L = lib()
    ws = torch.empty(L.scda_bias_grad_workspace_bytes(C) // 4, dtype=torch.float32, device=dy.device)
    _check(L.scda_bias_grad_nchw_hip(_p(dy), _p(db), B, C, HW, 0 if out is None else 1, _p(ws), _stream()), "scda_bias_grad_nchw_hip")
    return db


def colsum(dy, out=None):
    _req(dy, "dy")
    M, N = dy.shape
    db = out if out is not None else torch.empty(N, dtype=torch.float32, device=dy.device)
    _check(lib().scda_colsum_hip(_p(dy), _p(db), M, N, 0 if out is None else 1, _stream()), "scda_colsum_hip")
    return db


def softmax_ce_fwd(logits, targets, ignore_index=-100):
    _req(logits, "logits"); _req(targets, "targets", torch.int64)
    if logits.dim() != 2:
        raise ValueError("logits must be [R,C]")
    R, C = logits.shape
    if targets.numel() != R:
        raise ValueError(f"targets must hold one class per row ({R}), got {targets.numel()}")
    probs = torch.empty_like(logits)
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    _check(lib().scda_softmax_ce_fwd_hip(_p(logits), _p(targets), R, C, ignore_index, _p(probs), _p(out2), _stream()),
           "scda_softmax_ce_fwd_hip")
    return out2, probs


def softmax_ce_bwd(probs, targets, out2, g, ignore_index=-100):
    _req(probs, "probs"); _req(targets, "targets", torch.int64); _req(out2, "out2"); _req(g, "g")
    if probs.dim() != 2:
        raise ValueError("probs must be [R,C]")
    R, C = probs.shape
    if targets.numel() != R:
        raise ValueError(f"targets must hold one class per row ({R}), got {targets.numel()}")
    if out2.numel() != 2 or g.numel() != 1:
        raise ValueError("out2 must hold two values and g one")
    dx = torch.empty_like(probs)
    _check(lib().scda_softmax_ce_bwd_hip(_p(probs), _p(targets), R, C, ignore_index, _p(out2), _p(g), _p(dx), _stream()),
           "scda_softmax_ce_bwd_hip")
    return dx


def row_softmax(x):
    _req(x, "x")
    R, C = x.shape
    y = torch.empty_like(x)
    _check(lib().scda_row_softmax_hip(_p(x), _p(y), R, C, _stream()), "scda_row_softmax_hip")
    return y


def accuracy(logits, targets, ignore_index=-1):
    _req(logits, "logits"); _req(targets, "targets", torch.int64)
    R, C = logits.shape
    out = torch.empty(1, dtype=torch.float32, device=logits.device)
    _check(lib().scda_accuracy_hip(_p(logits), _p(targets), R, C, ignore_index, _p(out), _stream()), "scda_accuracy_hip")
    return out


def _req_smooth_l1(pred, mask, target):
    _req(pred, "pred"); _req(target, "target")
    if target.shape != pred.shape:
        raise ValueError(f"target must have the shape of pred {tuple(pred.shape)}, got {tuple(target.shape)}")
    if mask is not None:
        _req(mask, "mask")
        if mask.shape != pred.shape:
            raise ValueError(f"mask must have the shape of pred {tuple(pred.shape)}, got {tuple(mask.shape)}")


def smooth_l1_fwd(pred, mask, target, sigma, scale):
    _req_smooth_l1(pred, mask, target)
    L = lib()
    ws = torch.empty(L.scda_smooth_l1_workspace_bytes() // 4, dtype=torch.float32, device=pred.device)
    out = torch.empty(1, dtype=torch.float32, device=pred.device)
    _check(L.scda_smooth_l1_fwd_hip(_p(pred), _p(mask), _p(target), pred.numel(), sigma, scale, _p(ws), _p(out), _stream()),
           "scda_smooth_l1_fwd_hip")
    return out


def smooth_l1_bwd(pred, mask, target, sigma, scale, g):
    _req_smooth_l1(pred, mask, target); _req(g, "g")
    if g.numel() != 1:
        raise ValueError("g must hold one value")
    dp = torch.empty_like(pred)
    _check(lib().scda_smooth_l1_bwd_hip(_p(pred), _p(mask), _p(target), pred.numel(), sigma, scale, _p(g), _p(dp), _stream()),
           "scda_smooth_l1_bwd_hip")
    return dp


def instnorm_fwd(x, eps, act, slope):
    _req(x, "x")
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B * C, dtype=torch.float32, device=x.device)
    _check(lib().scda_instnorm_fwd_hip(_p(x), _p(y), _p(mean), _p(rstd), B * C, H * W, eps, act, slope, _stream()), "scda_instnorm_fwd_hip")
    return y, mean, rstd


def instnorm_bwd(dy, x, mean, rstd, act, slope):
    B, C, H, W = _req_map(x)
    _req_like(dy, "dy", x, "x")
    _req_channels(B * C, mean=mean, rstd=rstd)
    dx = torch.empty_like(x)
    _check(lib().scda_instnorm_bwd_hip(_p(dy), _p(x), _p(mean), _p(rstd), _p(dx), B * C, H * W, act, slope, _stream()),
           "scda_instnorm_bwd_hip")
    return dx


def instnorm_drop_add_fwd(x, residual, eps, p, seed):
    """residual + dropout_{p,seed}(instance_norm(x)) in one launch -> (y, mean, rstd)"""
    _req(x, "x"); _req(residual, "residual")
    if residual.shape != x.shape:
        raise ValueError("residual must have the shape of x")
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B * C, dtype=torch.float32, device=x.device)
    if torch.is_tensor(seed):     # a slot of a scda_amd.seeds.SeedArena: the kernel reads the seed from device memory
        _req(seed, "seed", torch.int64)
        _check(lib().scda_instnorm_drop_add_fwd_dev_hip(_p(x), _p(residual), _p(y), _p(mean), _p(rstd), B * C, H * W, eps, p, _p(seed),
                                                        1.0 / (1.0 - p), _stream()), "scda_instnorm_drop_add_fwd_dev_hip")
        return y, mean, rstd
    _check(lib().scda_instnorm_drop_add_fwd_hip(_p(x), _p(residual), _p(y), _p(mean), _p(rstd), B * C, H * W, eps, p,
                                                seed & 0xFFFFFFFFFFFFFFFF, 1.0 / (1.0 - p), _stream()), "scda_instnorm_drop_add_fwd_hip")
    return y, mean, rstd


def instnorm_drop_bwd(dy, x, mean, rstd, p, seed):
    _req(dy, "dy"); _req(x, "x")
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    if torch.is_tensor(seed):
        _check(lib().scda_instnorm_drop_bwd_dev_hip(_p(dy), _p(x), _p(mean), _p(rstd), _p(dx), B * C, H * W, p, _p(seed), 1.0 / (1.0 - p),
                                                    _stream()), "scda_instnorm_drop_bwd_dev_hip")
        return dx
    _check(lib().scda_instnorm_drop_bwd_hip(_p(dy), _p(x), _p(mean), _p(rstd), _p(dx), B * C, H * W, p, seed & 0xFFFFFFFFFFFFFFFF,
                                            1.0 / (1.0 - p), _stream()), "scda_instnorm_drop_bwd_dev_hip")
    return dx


def _bn_ws(B, C, HW, device):
    L = lib()
    n = L.scda_batchnorm_workspace_bytes(B, C, HW)
    return torch.empty(n // 4, dtype=torch.float32, device=device) if n else None


def batchnorm_fwd(x, gamma, beta, run_mean, run_var, eps, momentum, act, slope):
    B, C, H, W = _req_map(x)
    if gamma is None or beta is None:
        raise TypeError("batchnorm_fwd: gamma and beta must be tensors")
    _req_channels(C, gamma=gamma, beta=beta, running_mean=run_mean, running_var=run_var)
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = _bn_ws(B, C, H * W, x.device)
    _check(lib().scda_batchnorm_fwd_hip(_p(x), _p(y), _p(gamma), _p(beta), _p(run_mean), _p(run_var), _p(mean), _p(rstd), B, C, H * W, eps,
                                        momentum, act, slope, _p(ws), _stream()), "scda_batchnorm_fwd_hip")
    return y, mean, rstd


def batchnorm_bwd(dy, x, gamma, beta, mean, rstd, act, slope, need_dx=True, out=None):
    """out = (dgamma, dbeta) buffers to accumulate into, or None to allocate"""
    B, C, H, W = _req_map(x)
    _req_like(dy, "dy", x, "x")
    if any(v is None for v in (gamma, beta, mean, rstd)):
        raise TypeError("batchnorm_bwd: gamma, beta, mean and rstd must be tensors")
    _req_channels(C, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
    if out is not None:
        _req_channels(C, dgamma=out[0], dbeta=out[1])
    dx = torch.empty_like(x) if need_dx else None
    dg, db = out if out is not None else (torch.empty(C, dtype=torch.float32, device=x.device),
                                          torch.empty(C, dtype=torch.float32, device=x.device))
    _check(lib().scda_batchnorm_bwd_hip(_p(dy), _p(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), B, C, H * W, act,
                                        slope, 0 if out is None else 1, _p(_bn_ws(B, C, H * W, x.device)), _stream()),
           "scda_batchnorm_bwd_hip")
    return dx, dg, db


def batchnorm_add_relu_ok(x):
    """is relu(bn(x) + residual) served as one kernel for this map?  (batch 1, plane of a multiple of 4 up to 40960 elements)"""
    B, C, H, W = x.shape
    return bool(lib().scda_batchnorm_add_relu_ok(B, H * W))


def aligned16(*tensors):
    """the 16-byte alignment the plane kernels' float4 accesses need (a contiguous but OFFSET view -- a sliced residual, a dy that
    autograd hands over as a storage-offset view -- is contiguous and still not aligned)"""
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def batchnorm_add_relu_fwd(x, residual, gamma, beta, run_mean, run_var, eps, momentum):
    B, C, H, W = _req_map(x)
    _req(residual, "residual")
    if residual.shape != x.shape:
        raise ValueError("batchnorm_add_relu_fwd: shape mismatch")
    if gamma is None or beta is None:
        raise TypeError("batchnorm_add_relu_fwd: gamma and beta must be tensors")
    _req_channels(C, gamma=gamma, beta=beta, running_mean=run_mean, running_var=run_var)
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(C, dtype=torch.float32, device=x.device)
    _check(lib().scda_batchnorm_add_relu_fwd_hip(_p(x), _p(residual), _p(y), _p(gamma), _p(beta), _p(run_mean), _p(run_var), _p(mean),
                                                 _p(rstd), B, C, H * W, eps, momentum, _stream()), "scda_batchnorm_add_relu_fwd_hip")
    return y, mean, rstd


def batchnorm_add_relu_bwd(dy, x, y, gamma, beta, mean, rstd, need_dx=True, out=None):
    """-> (dx, d_residual, dgamma, dbeta); out = (dgamma, dbeta) buffers to accumulate into, or None to allocate"""
    B, C, H, W = _req_map(x)
    _req_like(dy, "dy", x, "x"); _req_like(y, "y", x, "x")
    if any(v is None for v in (gamma, beta, mean, rstd)):
        raise TypeError("batchnorm_add_relu_bwd: gamma, beta, mean and rstd must be tensors")
    _req_channels(C, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
    if out is not None:
        _req_channels(C, dgamma=out[0], dbeta=out[1])
    dx = torch.empty_like(x) if need_dx else None
    dres = torch.empty_like(x)
    dg, db = out if out is not None else (torch.empty(C, dtype=torch.float32, device=x.device),
                                          torch.empty(C, dtype=torch.float32, device=x.device))
    _check(lib().scda_batchnorm_add_relu_bwd_hip(_p(dy), _p(x), _p(y), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx), _p(dres), _p(dg),
                                                 _p(db), B, C, H * W, 0 if out is None else 1, _stream()),
           "scda_batchnorm_add_relu_bwd_hip")
    return dx, dres, dg, db


def batchnorm_eval(x, gamma, beta, run_mean, run_var, eps, act, slope, dy=None):
    """eval-mode batch norm (+act); with dy: the gradient w.r.t. x"""
    B, C, H, W = _req_map(x)
    if any(v is None for v in (gamma, beta, run_mean, run_var)):
        raise TypeError("batchnorm_eval: gamma, beta and the running statistics must be tensors")
    _req_channels(C, gamma=gamma, beta=beta, running_mean=run_mean, running_var=run_var)
    if dy is not None:
        _req_like(dy, "dy", x, "x")
    out = torch.empty_like(x)
    _check(lib().scda_batchnorm_eval_hip(_p(x), _p(dy), _p(out), _p(gamma), _p(beta), _p(run_mean), _p(run_var), B, C, H * W, eps, act,
                                         slope, _stream()), "scda_batchnorm_eval_hip")
    return out


def upsample2x_fwd(x):
    _req(x, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, C, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
    _check(lib().scda_upsample2x_fwd_hip(_p(x), _p(y), B * C, H, W, _stream()), "scda_upsample2x_fwd_hip")
    return y


def instnorm_up2_ok(x):
    """instance norm + the bilinear x2 behind it can run as one launch on this tensor (scda_instnorm_up2_supported + alignment)"""
    return (x.dim() == 4 and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and aligned16(x)
            and bool(lib().scda_instnorm_up2_supported(x.shape[2], x.shape[3])))


def instnorm_up2_fwd(x, eps, act, slope):
    """upsample2x(act(instance_norm(x))) in one launch -> (y2 [B, C, 2H, 2W], mean, rstd)"""
    _req(x, "x")
    B, C, H, W = x.shape
    y2 = torch.empty(B, C, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
    mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B * C, dtype=torch.float32, device=x.device)
    _check(lib().scda_instnorm_up2_fwd_hip(_p(x), _p(y2), _p(mean), _p(rstd), B * C, H, W, eps, act, slope, _stream()),
           "scda_instnorm_up2_fwd_hip")
    return y2, mean, rstd


def instnorm_drop_add_up2_fwd(x, residual, eps, p, seed):
    """upsample2x(residual + dropout_{p,seed}(instance_norm(x))) in one launch -> (y2, mean, rstd)"""
    _req(x, "x"); _req(residual, "residual")
    if residual.shape != x.shape:
        raise ValueError("residual must have the shape of x")
    B, C, H, W = x.shape
    y2 = torch.empty(B, C, 2 * H, 2 * W, dtype=torch.float32, device=x.device)
    mean = torch.empty(B * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B * C, dtype=torch.float32, device=x.device)
    if torch.is_tensor(seed):     # a slot of a scda_amd.seeds.SeedArena (see instnorm_drop_add_fwd)
        _req(seed, "seed", torch.int64)
        _check(lib().scda_instnorm_drop_add_up2_fwd_dev_hip(_p(x), _p(residual), _p(y2), _p(mean), _p(rstd), B * C, H, W, eps, p, _p(seed),
                                                            1.0 / (1.0 - p), _stream()), "scda_instnorm_drop_add_up2_fwd_dev_hip")
        return y2, mean, rstd
    _check(lib().scda_instnorm_drop_add_up2_fwd_hip(_p(x), _p(residual), _p(y2), _p(mean), _p(rstd), B * C, H, W, eps, p,
                                                    seed & 0xFFFFFFFFFFFFFFFF, 1.0 / (1.0 - p), _stream()),
           "scda_instnorm_drop_add_up2_fwd_hip")
    return y2, mean, rstd


def instnorm_up2_bwd(dy2, x, mean, rstd, act, slope):
    """gradient of instnorm_up2_fwd w.r.t. x: the bilinear gather and the norm's backward in one launch"""
    _req(dy2, "dy2"); _req(x, "x")
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    _check(lib().scda_instnorm_up2_bwd_hip(_p(dy2), _p(x), _p(mean), _p(rstd), _p(dx), B * C, H, W, act, slope, _stream()),
           "scda_instnorm_up2_bwd_hip")
    return dx


def instnorm_drop_up2_bwd(dy2, x, mean, rstd, p, seed):
    """gradients of instnorm_drop_add_up2_fwd -> (dx, dresidual): dresidual = the gathered gradient of the small plane"""
    _req(dy2, "dy2"); _req(x, "x")
    B, C, H, W = x.shape
    dx = torch.empty_like(x)
    dres = torch.empty_like(x)
    if torch.is_tensor(seed):
        _check(lib().scda_instnorm_drop_up2_bwd_dev_hip(_p(dy2), _p(x), _p(mean), _p(rstd), _p(dx), _p(dres), B * C, H, W, p, _p(seed),
                                                        1.0 / (1.0 - p), _stream()), "scda_instnorm_drop_up2_bwd_dev_hip")
        return dx, dres
    _check(lib().scda_instnorm_drop_up2_bwd_hip(_p(dy2), _p(x), _p(mean), _p(rstd), _p(dx), _p(dres), B * C, H, W, p,
                                                seed & 0xFFFFFFFFFFFFFFFF, 1.0 / (1.0 - p), _stream()), "scda_instnorm_drop_up2_bwd_hip")
    return dx, dres


def upsample2x_bwd(dy):
    _req(dy, "dy")
    B, C, OH, OW = dy.shape
    dx = torch.empty(B, C, OH // 2, OW // 2, dtype=torch.float32, device=dy.device)
    _check(lib().scda_upsample2x_bwd_hip(_p(dy), _p(dx), B * C, OH // 2, OW // 2, _stream()), "scda_upsample2x_bwd_hip")
    return dx


def bce_fwd(p, t):
    _req(p, "p"); _req(t, "t")
    if p.numel() != t.numel():
        raise ValueError("bce: shape mismatch")
    out = torch.empty(1, dtype=torch.float32, device=p.device)
    _check(lib().scda_bce_fwd_hip(_p(p), _p(t), p.numel(), _p(out), _stream()), "scda_bce_fwd_hip")
    return out


def bce_bwd(p, t, g):
    _req(p, "p"); _req(t, "t"); _req(g, "g")
    if p.numel() != t.numel() or g.numel() != 1:
        raise ValueError("bce: shape mismatch")
    dp = torch.empty_like(p)
    _check(lib().scda_bce_bwd_hip(_p(p), _p(t), p.numel(), _p(g), _p(dp), _stream()), "scda_bce_bwd_hip")
    return dp


def avg2x2s1_fwd(x):
    _req(x, "x")
    B, C, H1, W1 = x.shape
    y = torch.empty(B, C, H1 - 1, W1 - 1, dtype=torch.float32, device=x.device)
    _check(lib().scda_avg2x2s1_fwd_hip(_p(x), _p(y), B * C, H1 - 1, W1 - 1, _stream()), "scda_avg2x2s1_fwd_hip")
    return y


def avg2x2s1_bwd(dy):
    _req(dy, "dy")
    B, C, H, W = dy.shape
    dx = torch.empty(B, C, H + 1, W + 1, dtype=torch.float32, device=dy.device)
    _check(lib().scda_avg2x2s1_bwd_hip(_p(dy), _p(dx), B * C, H, W, _stream()), "scda_avg2x2s1_bwd_hip")
    return dx


def gap_fwd(x):
    _req(x, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, C, dtype=torch.float32, device=x.device)
    _check(lib().scda_gap_fwd_hip(_p(x), _p(y), B * C, H * W, _stream()), "scda_gap_fwd_hip")
    return y


def gap_bwd(dy, x_shape):
    _req(dy, "dy")
    B, C, H, W = x_shape
    dx = torch.empty(B, C, H, W, dtype=torch.float32, device=dy.device)
    _check(lib().scda_gap_bwd_hip(_p(dy), _p(dx), B * C, H * W, _stream()), "scda_gap_bwd_hip")
    return dx


def row_mean(x):
    _req(x, "x")
    R, C = x.shape
    y = torch.empty(R, dtype=torch.float32, device=x.device)
    _check(lib().scda_row_mean_hip(_p(x), _p(y), R, C, _stream()), "scda_row_mean_hip")
    return y


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, max_blocks=0):
    _req(param, "param"); _req(grad, "grad"); _req(exp_avg, "exp_avg"); _req(exp_avg_sq, "exp_avg_sq")
    _check(lib().scda_adam_limited_hip(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), lr, beta1, beta2, eps, weight_decay,
                                       step, max_blocks, _stream()), "scda_adam_hip")


def last_plan():
    """(tile rows, tile cols, split-K count, direct-to-LDS?) of this thread's most recent conv / GEMM launch; the last entry is the
    integer 2 (truthy) when the dense GEMM ran as the exact-product bf16 x 9 kernel"""
    out = (ctypes.c_int * 4)()
    lib().scda_debug_last_plan(out)
    return out[0], out[1], out[2], (2 if out[3] == 2 else bool(out[3]))


PLAN_FIELDS = ("family", "x9_stream", "bm", "bn", "splits", "k_per_split", "nx", "ny", "grid", "swz", "parity", "nc", "ncp", "wbk",
               "reduce", "x9_r")


def plan_conv(direction, batch, cin, ih, iw, cout, k, stride, pad, row_period=0, aligned=True, ws_bytes=None):
    """the launch decision (PLAN_FIELDS, see scda_ops.h) of a convolution: direction "fwd" | "dgrad" | "wgrad" | "wgrad_bias".  No GPU
    needed; ws_bytes defaults to what the operators pass (scda_conv2d_workspace_bytes)"""
    L = lib()
    if ws_bytes is None:
        ws_bytes = L.scda_conv2d_workspace_bytes(batch, cin, ih, iw, cout, k, k, stride, pad)
    out = (ctypes.c_int * 16)()
    L.scda_debug_plan_conv(("fwd", "dgrad", "wgrad", "wgrad_bias").index(direction), batch, cin, ih, iw, cout, k, k, stride, pad,
                           row_period, int(aligned), ws_bytes, out)
    return dict(zip(PLAN_FIELDS, out))


def plan_gemm(M, N, K, lda, ldb, trans_a=False, trans_b=False, aligned=True, ws_bytes=None, ldc=None):
    """the launch decision of a dense GEMM as gemm() would issue it, for a 256-CU device.  No GPU needed"""
    if ws_bytes is None:      # scda_gemm_workspace_bytes at 256 CUs (the entry itself asks the device)
        ws_bytes = max(16 * M * N * 4, 2 * 256 * 256 * 128 * 4)
    out = (ctypes.c_int * 16)()
    lib().scda_debug_plan_gemm(M, N, K, lda, ldb, N if ldc is None else ldc, int(trans_a), int(trans_b), int(aligned), ws_bytes, out)
    return dict(zip(PLAN_FIELDS, out))


WINO_PLAN_FIELDS = ("mb", "pixel_major", "gm", "splits", "slabs_per_split", "per_xcd", "n_wg", "persist", "epi")
WINO_WGRAD_PLAN_FIELDS = ("n_slab", "splits", "slabs_per_split", "splits_per_xcd", "order", "grid")


def plan_wino(kind, batch, cin, ih, iw, cout, row_period=0, ws_bytes=None):
    """the launch decision of a stride-1 pad-1 3x3 layer on the Winograd kernels, for a 256-CU device (no GPU needed): kind "fwd" |
    "fwd_pool" | "dgrad" | "dgrad_mask" -> WINO_PLAN_FIELDS, "wgrad" | "wgrad_bias" -> WINO_WGRAD_PLAN_FIELDS.  ws_bytes defaults to
    what the operators pass"""
    L = lib()
    if ws_bytes is None:
        ws_bytes = 0 if kind == "fwd_pool" else L.scda_conv2d_workspace_bytes(batch, cin, ih, iw, cout, 3, 3, 1, 1)
    C, M = (cout, cin) if kind.startswith("dgrad") else (cin, cout)      # the data gradient reduces over Cout
    fwd, wgrad = (ctypes.c_int * 9)(), (ctypes.c_int * 6)()
    L.scda_debug_plan_wino(batch, C, ih, iw, M, wino_stacked(batch, ih, iw, row_period), int(kind == "fwd_pool"), int(kind == "dgrad_mask"),
                           int(kind == "wgrad_bias"), ws_bytes, fwd, wgrad)
    return dict(zip(WINO_WGRAD_PLAN_FIELDS, wgrad)) if kind.startswith("wgrad") else dict(zip(WINO_PLAN_FIELDS, fwd))


def wino_last_persistent():
    """was this thread's most recent Winograd forward / data-gradient launch the persistent form (one workgroup per CU walking the tiles)?"""
    return bool(lib().scda_debug_wino_last_persistent())


def wino_last_order():
    """launch order of this thread's most recent Winograd launches: ((tile rows / 32, pixel-block-major?, gm, splits), (wgrad splits, wgrad order))"""
    out = (ctypes.c_int * 6)()
    lib().scda_debug_wino_last_order(out)
    return (out[0], bool(out[1]), out[2], out[3]), (out[4], out[5])


# ------------------------------------------------------------ profiler ------
def prof_kernel_names():
    L = lib()
    return [L.scda_prof_kernel_name(k).decode() for k in range(L.scda_prof_num_kernels())]


def prof_enable(kernels):
    """kernels: False/None = off, True = all GEMM-class kernels, or an iterable of kernel names to time"""
    names = prof_kernel_names()
    if not kernels:
        mask = 0
    elif kernels is True:
        mask = (1 << len(names)) - 1
    else:
        mask = 0
        for k in kernels:
            mask |= 1 << names.index(k)
    lib().scda_prof_enable(mask)


def prof_collect():
    """after torch.cuda.synchronize(): {kernel name: (launches, total_ms, total_flops, total_algorithmic_bytes)} for the
    kernel classes that ran"""
    L = lib()
    n = L.scda_prof_num_kernels()
    launches = (ctypes.c_longlong * n)()
    ms = (ctypes.c_double * n)()
    fl = (ctypes.c_double * n)()
    by = (ctypes.c_double * n)()
    _check(L.scda_prof_collect(launches, ms, fl, by), "scda_prof_collect")
    return {L.scda_prof_kernel_name(k).decode(): (int(launches[k]), float(ms[k]), float(fl[k]),
                                                  float(by[k])) for k in range(n) if launches[k] > 0}


# ------------------------------------------------------------ data path -----
def image_resize_normalize(src, tables, out_h, out_w, normalize=True, mean=0.5, std=0.5, flip=False):
    """src uint8 [H, W, C] (device) -> float32 [C, out_h, out_w]: PIL resize + optional flip + ToTensor + Normalize on the device
    (scda_image_resize_normalize_hip; datasets/example_dataset.py:76-131).  `tables` = (bounds_h, kk_h, ksize_h, bounds_v, kk_v,
    ksize_v, row0, rows): device int32 tensors and ints from device_image.resize_tables."""
    _req(src, "src", torch.uint8)
    H, W, C = src.shape
    bh, kh, ksh, bv, kv, ksv, row0, rows = tables
    for t, name in ((bh, "bounds_h"), (kh, "kk_h"), (bv, "bounds_v"), (kv, "kk_v")):
        _req(t, name, torch.int32)
    L = lib()
    nb = int(L.scda_image_resize_tmp_bytes(rows, out_w, C))
    tmp = torch.empty(nb, dtype=torch.uint8, device=src.device)
    out = torch.empty(C, out_h, out_w, dtype=torch.float32, device=src.device)
    _check(L.scda_image_resize_normalize_hip(_p(src), H, W, C, _p(bh), _p(kh), ksh, out_w, _p(bv), _p(kv), ksv, out_h, row0, rows, _p(tmp),
                                             nb, 1 if normalize else 0, mean, std, 1 if flip else 0, _p(out), _stream()),
           "scda_image_resize_normalize_hip")
    return out


# ------------------------------------------------------- host -> device ------
def upload(array_or_tensor, device, dtype=None):
    """numpy array / CPU tensor -> device tensor through a pinned staging buffer with a non-blocking copy.
    (`tensor.to(device)` from pageable memory is a synchronous, stream-ordered hipMemcpy: the host would sit behind
    every kernel already queued on the stream.)"""
    t = array_or_tensor if isinstance(array_or_tensor, torch.Tensor) else torch.from_numpy(array_or_tensor)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    pin = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    pin.copy_(t)
    return pin.to(device, non_blocking=True)
