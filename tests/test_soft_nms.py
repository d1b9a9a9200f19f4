"""Soft-NMS at test time, the part that needs no GPU: the host loop of cython_nms.soft_nms against the reference's compiled soft_nms
on every fixture case (tests/golden/soft_nms_ref.npz: lengths 1 .. 2048, float and integer coordinates, untied scores and scores in
eighths, three methods, three parameter sets) -- the rule set the HIP kernel is judged by in tests/test_soft_nms_gpu.py --, the
`soft_nms` key of test_predict_bbox_cfg through compute_predicted_bboxes, the setting's validation and the C ABI's declarations."""
import os

import numpy as np
import pytest
import torch

import soft_nms_cases as sc
import soft_nms_refs as refs
from test_host_functions import CFG, cpu_backend  # noqa: F401  (the fixture that points the NMS hook at the C oracle)


@pytest.fixture(scope="module")
def fixture_cases(golden_dir):
    return sc.load(os.path.join(golden_dir, "soft_nms_ref.npz"))


def test_fixture_covers_the_case_grid(fixture_cases):
    assert sorted(fixture_cases) == [(m, p) for m in (0, 1, 2) for p in (0, 1, 2)]
    for (m, p), cases in fixture_cases.items():
        names = [c[0] for c in cases]
        want = [sc.name_of(n, i, t) for n in sc.SIZES for i in (False, True) for t in (False, True) if n != sc.BIG or (m, p) == sc.BIG_AT]
        assert names == want
    assert any(c[0].startswith("n2048_") for c in fixture_cases[sc.BIG_AT])


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("pi", range(len(sc.PARAMS)))
def test_host_loop_equals_reference_bit_for_bit(fixture_cases, method, pi):
    from scda_amd.dropin.extensions._cython_bbox import cython_nms
    sigma, Nt, threshold = sc.PARAMS[pi]
    for name, dets, want_boxes, want_inds in fixture_cases[(method, pi)]:
        before = dets.copy()
        boxes, inds = cython_nms.soft_nms(dets, sigma, Nt, threshold, method)
        assert np.array_equal(dets.view(np.uint32), before.view(np.uint32)), name            # works on a copy, like the reference
        np.testing.assert_array_equal(np.asarray(inds), want_inds, err_msg=name)
        assert boxes.dtype == np.float32
        np.testing.assert_array_equal(boxes.view(np.uint32), want_boxes.view(np.uint32), err_msg=name)


def _head():
    rois, counts, prob, loc, info = refs.synth_head(seed=3)
    real = refs.real_rows(counts, 64)
    return rois[real], prob[real], loc[real], info


@pytest.mark.parametrize("method", [0, 1, 2])
def test_compute_predicted_bboxes_with_the_soft_nms_key(cpu_backend, method):  # noqa: F811
    """the eval forward's predict_bbox_fn with the cfg key set = the plain numpy composition, row for row and bit for bit"""
    from scda_amd.dropin.functions.predict_bbox import compute_predicted_bboxes
    soft = dict(refs.SETTINGS[1], method=('hard', 'linear', 'gaussian')[method])
    cfg = dict(CFG["test_predict_bbox_cfg"], score_thresh=0.05, top_n=40, soft_nms=soft)
    rois, prob, loc, info = _head()
    got = compute_predicted_bboxes(torch.from_numpy(rois), torch.from_numpy(prob), torch.from_numpy(loc), info, cfg).numpy()
    want = refs.predict_rows(rois, prob, loc, info, cfg, soft)
    assert got.dtype == np.float32 and got.shape == want.shape and set(got[:, 0]) == {0.0, 1.0}
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not (got[:, 6] == 2).any() and len(np.unique(got[:, 6])) == 2                        # the empty class gives no row
    if method:                                                                                  # rescored: not the head's scores
        assert not np.isin(got[:, 5], prob).all()


def test_compute_predicted_bboxes_without_the_key_is_unchanged(cpu_backend, golden_dir):  # noqa: F811
    """no key, or None: the rows of the reference's golden output, byte for byte, as before"""
    from scda_amd.dropin.functions.predict_bbox import compute_predicted_bboxes
    g = np.load(os.path.join(golden_dir, "predict_bbox.npz"))
    for cfg in (CFG["test_predict_bbox_cfg"], dict(CFG["test_predict_bbox_cfg"], soft_nms=None)):
        bb = compute_predicted_bboxes(torch.from_numpy(g["rois"]), torch.from_numpy(g["pred_cls"]), torch.from_numpy(g["pred_loc"]),
                                      g["image_info"], cfg)
        assert bb.numpy().tobytes() == np.ascontiguousarray(g["bboxes"]).tobytes()
    # and on the synthetic head a cfg with the key gives OTHER rows than one without: the key is what switches
    rois, prob, loc, info = _head()
    cfg = dict(CFG["test_predict_bbox_cfg"], score_thresh=0.05, top_n=40)
    hard = compute_predicted_bboxes(torch.from_numpy(rois), torch.from_numpy(prob), torch.from_numpy(loc), info, cfg).numpy()
    soft = compute_predicted_bboxes(torch.from_numpy(rois), torch.from_numpy(prob), torch.from_numpy(loc), info,
                                    dict(cfg, soft_nms=refs.SETTINGS[2])).numpy()
    assert hard.shape != soft.shape or not np.array_equal(hard, soft)


def test_backend_soft_nms_segments_with_a_substituted_hook(cpu_backend, fixture_cases):  # noqa: F811
    from scda_amd.dropin import backend
    cases = fixture_cases[(1, 0)][:24]                                  # lengths 1 .. 128
    lists = [c[1] for c in cases] + [np.zeros((0, 5), dtype=np.float32)]
    got = backend.soft_nms_segments(lists, 1, *sc.PARAMS[0])
    assert len(got) == len(lists) and got[-1][0].shape == (0, 5) and got[-1][1].shape == (0,)
    for (name, _, want_boxes, want_inds), (boxes, inds) in zip(cases, got):
        np.testing.assert_array_equal(inds, want_inds, err_msg=name)
        np.testing.assert_array_equal(boxes.view(np.uint32), want_boxes.view(np.uint32), err_msg=name)


def test_setting_validation():
    from scda_amd import native as N
    assert N.soft_nms_setting(None) is None
    assert N.soft_nms_setting({}) == (0, 0.5, 0.3, 0.001)               # the reference's defaults
    assert N.soft_nms_setting({'method': 'gaussian', 'sigma': 0.3}) == (2, 0.3, 0.3, 0.001)
    assert N.soft_nms_setting({'method': 1, 'Nt': 0.5, 'threshold': 0.05}) == (1, 0.5, 0.5, 0.05)
    for bad in ({'method': 'cubic'}, {'method': 3}, {'method': True}, {'sigma': 0}, {'sigma': -1.0}, {'nt': 0.3}, "linear"):
        with pytest.raises(ValueError):
            N.soft_nms_setting(bad)


class _Eval:
    training = False


def _cfg(post_nms_top_n=300, **box):
    cfg = {k: dict(v) for k, v in CFG.items()}
    cfg["test_rpn_proposal_cfg"]["post_nms_top_n"] = post_nms_top_n
    cfg["test_predict_bbox_cfg"].update(box)
    return cfg


def test_predictor_validates_the_setting():
    from scda_amd import infer
    from scda_amd import native as N
    cap = N.soft_nms_capacity()
    assert cap == 2048
    assert infer.Predictor(_Eval(), _cfg()).soft_nms is None
    assert infer.Predictor(_Eval(), _cfg(post_nms_top_n=cap + 1)).soft_nms is None              # the capacity binds the soft sweep only
    assert infer.Predictor(_Eval(), _cfg(soft_nms={'method': 'linear'})).soft_nms == (1, 0.5, 0.3, 0.001)      # from the cfg key
    assert infer.Predictor(_Eval(), _cfg(soft_nms={'method': 'linear'}), soft_nms={'method': 'gaussian', 'sigma': 0.4}).soft_nms \
        == (2, 0.4, 0.3, 0.001)                                                                 # the argument overrides the key
    assert infer.Predictor(_Eval(), _cfg(post_nms_top_n=cap), soft_nms={'method': 'hard'}).soft_nms[0] == 0
    for kw in ({'soft_nms': {'method': 'cubic'}}, {'soft_nms': {'method': 'gaussian', 'sigma': 0.0}}):
        with pytest.raises(ValueError):
            infer.Predictor(_Eval(), _cfg(), **kw)
    with pytest.raises(ValueError):
        infer.Predictor(_Eval(), _cfg(soft_nms={'method': 'quadratic'}))
    with pytest.raises(ValueError, match="2048"):
        infer.Predictor(_Eval(), _cfg(post_nms_top_n=cap + 1), soft_nms={'method': 'linear'})


def test_box_predict_validates_before_it_touches_the_device():
    """an unknown method or a P above the capacity is a ValueError on any machine: nothing is bound to a device, nothing launched"""
    from scda_amd import native as N
    C, top_n = 3, 5

    def call(P, soft):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)      # noqa: E731
        return N.box_predict(z(P, 5), z(1, dt=torch.int32), z(P, C), z(P, 4 * C), z(1, 3), [0.1, 0.1, 0.2, 0.2], [0, 0, 0, 0], 0.0, 0.5,
                             top_n, z(8, dt=torch.uint8), z(1, top_n, 7), z(1, dt=torch.int32), soft_nms=soft)
    with pytest.raises(ValueError, match="method"):
        call(8, {'method': 'cubic'})
    with pytest.raises(ValueError, match="2048"):
        call(N.soft_nms_capacity() + 1, {'method': 'linear'})
    with pytest.raises(N.ScdaNativeError):                              # a valid setting gets as far as the device check
        call(8, {'method': 'linear'})


def test_header_declares_the_entry_points():
    from scda_amd import native as N
    with open(N.HEADER_PATH) as f:
        sigs = N.parse_header(f.read())
    import ctypes
    v, i, fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert sigs["scda_soft_nms_segments_hip"] == (i, [v, v, i, i, i, fl, fl, fl, v, v, v])
    assert sigs["scda_soft_nms_capacity"] == (i, [])
    hard, soft = sigs["scda_box_predict_hip"], sigs["scda_box_predict_soft_hip"]
    assert soft[0] is i and len(soft[1]) == len(hard[1]) + 3            # nms_thresh leaves, (method, sigma, Nt, threshold) come
    assert soft[1][:12] == hard[1][:12] and soft[1][12:17] == [i, i, fl, fl, fl] and soft[1][17:] == hard[1][14:]
    lib = N.lib()
    for name in ("scda_soft_nms_segments_hip", "scda_soft_nms_capacity", "scda_box_predict_soft_hip"):
        assert getattr(lib, name).argtypes == sigs[name][1]
