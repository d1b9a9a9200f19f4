"""The C-ABI library loads, exports every symbol include/*.h declares and is bound with the header's own signatures (no compute, no
GPU)."""
import ctypes
import glob
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    names = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names += re.findall(r"\b(scda_\w+)\s*\(", src)
    return sorted(set(names))


def test_header_declares_entry_points():
    names = declared_symbols()
    assert len(names) >= 16
    for must in ("scda_nms_hip", "scda_roi_pool_fwd_hip", "scda_roi_pool_bwd_hip", "scda_roi_align_fwd_hip",
                 "scda_focal_sigmoid_fwd_hip", "scda_focal_softmax_bwd_hip", "scda_iou_overlaps_hip"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from scda_amd import native
    lib = native.lib()
    missing = [n for n in declared_symbols() if not hasattr(lib, n)]
    assert not missing, f"libscda_ops.so lacks: {missing}"
    assert lib.scda_version() >= 100


def declared_parameters():
    """{name: text between the parentheses of its declaration}: a reading of the header of its own, not the binder's parser"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scda_ops.h")).read(), flags=re.S)
    return dict(re.findall(r"\b(scda_\w+)\s*\(([^)]*)\)\s*;", src))


def test_every_declared_function_is_typed_with_its_parameter_count():
    from scda_amd import native
    lib = native.lib()
    counts = {name: 0 if params.strip() == "void" else params.count(",") + 1 for name, params in declared_parameters().items()}
    assert sorted(counts) == declared_symbols()
    for name, n in counts.items():
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None, name
        assert len(argtypes) == n, (name, len(argtypes), n)


def _param(name, param):
    """the argtype of the parameter called `param` in the header's declaration of `name`"""
    from scda_amd import native
    index = [re.sub(r"\[\d*\]", "", p).split()[-1].lstrip("*") for p in declared_parameters()[name].split(",")].index(param)
    return getattr(native.lib(), name).argtypes[index]


def test_binding_of_a_spread_of_signatures():
    from scda_amd import native
    lib = native.lib()
    assert lib.scda_nms_workspace_bytes.restype is ctypes.c_size_t
    assert lib.scda_conv2d_pack_tiles.restype is ctypes.c_longlong
    assert lib.scda_last_error.restype is ctypes.c_char_p
    assert lib.scda_prof_kernel_name.restype is ctypes.c_char_p
    assert lib.scda_debug_last_plan.restype is None
    assert lib.scda_nms_hip.restype is ctypes.c_int
    assert lib.scda_mask_select_hip.argtypes[1:5] == [ctypes.c_longlong] * 4      # parameters 2-5: the four strides
    assert lib.scda_mask_select_hip.argtypes[0] is ctypes.c_void_p and lib.scda_mask_select_hip.argtypes[6] is ctypes.c_int
    for name in ("scda_conv2d_fwd_hip", "scda_gemm_hip"):
        assert _param(name, "ws_bytes") is ctypes.c_size_t
        assert _param(name, "slope") is ctypes.c_float
    assert _param("scda_dropout_seeded_hip", "seed") is ctypes.c_uint64
    assert _param("scda_rpn_proposals_hip", "min_size") is ctypes.c_double
    assert _param("scda_box_predict_hip", "stds_host") is ctypes.c_void_p
    assert _param("scda_box_predict_hip", "means_host") is ctypes.c_void_p
    assert lib.scda_prof_enable.argtypes == [ctypes.c_uint]
    assert lib.scda_version.argtypes == []


def test_parser_on_fragments():
    from scda_amd import native
    sigs = native.parse_header("""
        #define X 1
        /* a multi-line declaration */
        size_t f(const float *a, /* the count,
                                    in elements */ long long n,
                 const double stds[4], uint64_t seed,
                 void *stream);
        const char *g(void);
        void h(unsigned mask, double d, float x, int *out4);
    """)
    V = ctypes.c_void_p
    assert sigs == {"f": (ctypes.c_size_t, [V, ctypes.c_longlong, V, ctypes.c_uint64, V]),
                    "g": (ctypes.c_char_p, []),
                    "h": (None, [ctypes.c_uint, ctypes.c_double, ctypes.c_float, V])}
    with pytest.raises(native.ScdaNativeError, match=r"scda_wide.*__int128"):
        native.parse_header("int scda_wide(int n, __int128 big);")
    with pytest.raises(native.ScdaNativeError, match="scda_ret"):
        native.parse_header("short scda_ret(int n);")
    with pytest.raises(native.ScdaNativeError, match="typedef"):
        native.parse_header("typedef int (*scda_cb)(int);")


def test_too_few_arguments_raise_before_the_call():
    from scda_amd import native
    with pytest.raises(TypeError):
        native.lib().scda_nms_workspace_bytes()
    with pytest.raises(ctypes.ArgumentError):
        native.lib().scda_nms_workspace_bytes(1.5)       # a float where an int is declared


def test_a_missing_header_fails_at_load(monkeypatch):
    from scda_amd import native
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(native.ScdaNativeError, match="no_such_header.h"):
        native.lib()


def test_product_has_no_cpu_fallback():
    """Calling an operator with CPU tensors must raise, not silently compute on the host."""
    import torch
    from scda_amd import native
    with pytest.raises(native.ScdaNativeError):
        native.nms(torch.zeros(4, 5), 0.5)
    with pytest.raises(native.ScdaNativeError):
        native.roi_pool_fwd(torch.zeros(1, 2, 4, 4), torch.zeros(1, 5), 7, 7, 1.0)


def test_product_does_not_import_oracle():
    bad = []
    for path in glob.glob(os.path.join(ROOT, "scda_amd", "**", "*.py"), recursive=True):
        src = open(path).read()
        if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "liboracle" in src:
            bad.append(path)
    assert not bad, f"product files reference the oracle: {bad}"
