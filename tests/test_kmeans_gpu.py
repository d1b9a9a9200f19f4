"""The cluster-region generator on the MI355X (scda_amd/csrc/cluster_ops.hip, scda_amd/device_clusters.py) against the fixtures of
tests/golden/kmeans_ref.npz (the reference's compute_cluster_targets and sklearn 1.7.2's KMeans, see tests/test_kmeans_rules.py)
and against tests/kmeans_np.py, the numpy statement of the same rule in the same summation order.
Seeds, labels, counts, member lists, n_iter and crop corners: equal.  Centres: within 1e-3 px of the fixtures (the bound
tests/test_host_functions.py gives the host path) and bit-equal to the numpy statement (same float64 operations in the same order)."""
import warnings

import numpy as np
import pytest
import torch

import kmeans_np as KN
from test_kmeans_rules import CENTRE_ATOL, EQUAL, FALLBACK, corners_of, rng_state_equals

pytestmark = pytest.mark.gpu


@pytest.fixture()
def host_calls(monkeypatch):
    """counts the calls of the sklearn path (functions/mask.py:host_cluster_targets): one per call with the switch off, and with the
    switch on one for every call that the device path hands back"""
    from scda_amd.dropin.functions import mask
    real, calls = mask.host_cluster_targets, [0]

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(mask, "host_cluster_targets", counted)
    return calls


def run_kernel(rois_np, k, dev, n_runs=1):
    """scda_kmeans_hip on the rows -> the outputs as numpy arrays (one dict per run)"""
    from scda_amd import device_clusters, native
    n = rois_np.shape[0]
    rois = torch.from_numpy(np.ascontiguousarray(rois_np, dtype=np.float32)).to(dev)
    first, uniforms, _ = device_clusters.seeding_constants(n, k) if 1 <= k <= 8 else (0, None, 0)
    outs = []
    for _ in range(n_runs):
        i32 = dict(dtype=torch.int32, device=dev)
        bufs = {"centres": torch.full((k, 2), -7.0, device=dev), "labels": torch.full((n,), -7, **i32), "counts": torch.full((k,), -7, **i32),
                "members": torch.full((k, n), -7, **i32), "seed_index": torch.full((k,), -7, **i32), "n_iter": torch.full((1,), -7, **i32),
                "status": torch.full((1,), -7, **i32)}
        native.kmeans(rois, k, first, uniforms, bufs)
        torch.cuda.synchronize()
        outs.append({key: v.cpu().numpy() for key, v in bufs.items()})
    return outs


@pytest.mark.parametrize("s", EQUAL, ids=[s["name"] for s in EQUAL])
def test_kernel_matches_fixtures(cuda, s):
    k, n = int(s["k"]), s["rois"].shape[0]
    out, = run_kernel(s["rois"], k, cuda)
    assert int(out["status"][0]) == 0
    np.testing.assert_array_equal(out["seed_index"], s["seed_index"])
    np.testing.assert_array_equal(out["labels"], s["labels"])
    counts = np.bincount(s["labels"], minlength=k)
    np.testing.assert_array_equal(out["counts"], counts)
    for c in range(k):                                    # ascending member lists, then -1
        np.testing.assert_array_equal(out["members"][c, :counts[c]], np.where(s["labels"] == c)[0])
        assert (out["members"][c, counts[c]:] == -1).all()
    assert int(out["n_iter"][0]) == int(s["n_iter"])
    np.testing.assert_allclose(out["centres"], s["centres"], rtol=0, atol=CENTRE_ATOL)
    np.testing.assert_array_equal(corners_of(out["centres"]), s["corners"])
    km = KN.kmeans(s["rois"], k)                          # the second statement: same operations, same order -> same bits
    np.testing.assert_array_equal(out["centres"].view(np.uint32), km["centres"].view(np.uint32))
    assert n <= KN.CAPACITY


def test_two_runs_are_bit_identical(cuda):
    for s in (EQUAL[0], [x for x in EQUAL if int(x["k"]) == 8][0]):
        a, b = run_kernel(s["rois"], int(s["k"]), cuda, n_runs=2)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key


def test_row_stride_and_extra_columns(cuda):
    """RoI rows with more than five columns (proposals carry a score): the stride is honoured"""
    s = EQUAL[0]
    wide = np.concatenate([s["rois"], np.full((s["rois"].shape[0], 2), 1e6, dtype=np.float32)], axis=1)
    a, = run_kernel(s["rois"], int(s["k"]), cuda)
    b, = run_kernel(wide, int(s["k"]), cuda)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize("s", FALLBACK, ids=[s["name"] for s in FALLBACK])
def test_fallback_class(cuda, s, monkeypatch, host_calls):
    """fewer than k distinct points: status bit 0, and the call ends as the host path does (here: the reference's ValueError for a
    finally-empty cluster), on the same state of the global generator"""
    from scda_amd.dropin.functions.mask import compute_cluster_targets
    k, thr, n = int(s["k"]), int(s["threshold"]), s["rois"].shape[0]
    out, = run_kernel(s["rois"], k, cuda)
    assert int(out["status"][0]) & 1
    assert int(s["raises"]) == 1
    feats = torch.arange(n, dtype=torch.float32, device=cuda)[:, None].repeat(1, 8)
    states = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("SCDA_DEVICE_KMEANS", switch)
        before = host_calls[0]
        np.random.seed(int(s["rng_seed"]))
        with warnings.catch_warnings(), pytest.raises(ValueError):
            warnings.simplefilter("ignore")               # sklearn's "fewer distinct clusters than n_clusters"
            compute_cluster_targets(torch.from_numpy(s["rois"]), feats, N_cluster=k, threshold=thr)
        states[switch] = np.random.get_state()
        assert host_calls[0] - before == 1                # (switch on: the kernel's status sends the call back to the sklearn path)
    assert np.array_equal(states["0"][1], states["1"][1]) and states["0"][2] == states["1"][2]


def test_short_buffers_are_refused_before_the_launch(cuda):
    """the wrapper checks every output buffer for dtype, device and size: a short or mistyped one never reaches the kernel"""
    from scda_amd import device_clusters, native
    n, k = 64, 4
    rois = torch.zeros(n, 5, device=cuda)
    first, uniforms, _ = device_clusters.seeding_constants(n, k)
    i32 = dict(dtype=torch.int32, device=cuda)
    good = {"centres": torch.zeros(k, 2, device=cuda), "labels": torch.zeros(n, **i32), "counts": torch.zeros(k, **i32),
            "members": torch.zeros(k, n, **i32), "seed_index": torch.zeros(k, **i32), "n_iter": torch.zeros(1, **i32), "status": torch.zeros(1, **i32)}
    for key, bad, err in (("members", torch.zeros(k, n - 1, **i32), ValueError), ("labels", torch.zeros(n - 1, **i32), ValueError),
                          ("centres", torch.zeros(k, device=cuda), ValueError), ("counts", torch.zeros(k, dtype=torch.int64, device=cuda), TypeError),
                          ("status", torch.zeros(1, dtype=torch.int32), native.ScdaNativeError)):
        with pytest.raises(err):
            native.kmeans(rois, k, first, uniforms, dict(good, **{key: bad}))
    with pytest.raises(ValueError):
        native.kmeans(rois, k, first, None, good)
    with pytest.raises(ValueError):
        native.kmeans(rois[:, :4].contiguous(), k, first, uniforms, good)


def test_bad_arguments_raise_status_bit_1(cuda):
    rois = np.zeros((KN.CAPACITY + 1, 5), dtype=np.float32)
    for r, k in ((rois, 4), (rois[:3], 4)):
        out, = run_kernel(r, k, cuda)
        assert int(out["status"][0]) == 2 and (out["labels"] == -7).all() and (out["members"] == -7).all()


@pytest.mark.parametrize("F", [4096, 2048, 10])
def test_gather_is_bit_equal_to_index_select(cuda, F):
    """[k, threshold, F] at the VGG (4096) and ResNet (2048) widths, and a width that takes the 4-byte path; with picks (clusters
    smaller than threshold) and without; contiguous and strided feature rows"""
    from scda_amd import native
    r = np.random.RandomState(F)
    n, k = 512, 4
    feats = torch.from_numpy(r.standard_normal((n, F + 4)).astype(np.float32)).to(cuda)
    labels = r.randint(0, k, n)
    labels[:40] = 3
    for thr in (64, 128, 200):                            # every cluster larger / mixed / every cluster smaller
        counts = np.bincount(labels, minlength=k)
        members = np.full((k, n), -1, dtype=np.int32)
        rows = np.zeros((k, thr), dtype=np.int64)
        picks = np.zeros((k, thr), dtype=np.int32)
        for c in range(k):
            m = np.where(labels == c)[0]
            members[c, :m.size] = m
            if m.size < thr:
                picks[c] = r.randint(0, m.size, thr)
                rows[c] = m[picks[c]]
            else:
                rows[c] = m[:thr]
        short = bool((counts < thr).any())
        assert short == (thr != 64)
        m_dev, c_dev = torch.from_numpy(members).to(cuda), torch.from_numpy(counts.astype(np.int32)).to(cuda)
        p_dev = torch.from_numpy(picks).to(cuda) if short else None
        flat = torch.from_numpy(rows.reshape(-1)).to(cuda)
        for src in (feats[:, :F].contiguous(), feats[:, :F] if F % 4 == 0 else feats[:, 1:F + 1]):
            got = native.cluster_gather(src, m_dev, c_dev, p_dev, k, thr)
            want = src.index_select(0, flat).view(k, thr, F)
            assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    # a pick outside its list, or no picks for a short cluster: a row of zeros, nothing read out of bounds
    bad = torch.full((k, 200), n + 5, dtype=torch.int32, device=cuda)
    for p in (bad, None):
        got = native.cluster_gather(feats[:, :F].contiguous(), m_dev, c_dev, p, k, 200)
        assert float(got.abs().max()) == 0.0


def _features(n, F, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, F, generator=g).to(dev)


@pytest.mark.parametrize("how", ["host_rows", "device_rows", "cpu_tensor"])
def test_switch_on_equals_switch_off(cuda, monkeypatch, how, host_calls):
    """compute_cluster_targets with SCDA_DEVICE_KMEANS=1 against the unchanged host path, same seeded global generator: features bit-equal,
    centres within the bound, corners equal, np.random.get_state() equal afterwards.  The RoIs arrive as the trainer hands them over
    (a device tensor with its host copy riding along), as a bare device tensor, and as a CPU tensor."""
    from scda_amd import device_clusters
    from scda_amd.dropin.functions.mask import compute_cluster_targets
    picked = [s for s in EQUAL if s["name"].split("_")[0] in ("padded", "count") or s["rois"].shape[0] in (96, 16)][::2] + EQUAL[:2]
    for s in picked:
        k, thr, n = int(s["k"]), int(s["threshold"]), s["rois"].shape[0]
        feats = _features(n, 4096 if n == 512 else 256, cuda, n + k)
        res = {}
        for switch in ("0", "1"):
            monkeypatch.setenv("SCDA_DEVICE_KMEANS", switch)
            assert device_clusters.enabled() == (switch == "1")
            rois = torch.from_numpy(s["rois"])
            if how != "cpu_tensor":
                rois = rois.to(cuda)
                if how == "host_rows":
                    rois._scda_host = s["rois"]
            before = host_calls[0]
            np.random.seed(int(s["rng_seed"]))
            cf, centres = compute_cluster_targets(rois, feats, N_cluster=k, threshold=thr)
            torch.cuda.synchronize()
            assert host_calls[0] - before == 1 - int(switch)   # switch on: the device path itself, not its way back to the host
            assert rng_state_equals(s), s["name"]
            assert cf.is_cuda and cf.dtype == torch.float32 and not cf.requires_grad and tuple(cf.shape) == (k, thr, feats.shape[1])
            assert isinstance(centres, np.ndarray) and centres.dtype == np.float32 and centres.shape == (k, 2)
            res[switch] = (cf, centres)
        assert torch.equal(res["1"][0].view(torch.int32), res["0"][0].view(torch.int32)), s["name"]
        np.testing.assert_array_equal(res["1"][0][:, :, 0].cpu().numpy(), feats[:, 0].cpu().numpy()[s["rows"].astype(np.int64)])
        np.testing.assert_allclose(res["1"][1], res["0"][1], rtol=0, atol=CENTRE_ATOL)
        np.testing.assert_array_equal(corners_of(res["1"][1]), corners_of(res["0"][1]))


def test_over_capacity_takes_the_host_path(cuda, monkeypatch, host_calls):
    """N = capacity + 1 (and k = 9): the unchanged sklearn path answers, on the same state of the global generator"""
    from scda_amd import native
    from scda_amd.dropin.functions.mask import compute_cluster_targets
    n = native.kmeans_capacity() + 1
    assert n == KN.CAPACITY + 1
    r = np.random.RandomState(11)
    x1, y1 = r.uniform(0, 900, n), r.uniform(0, 400, n)
    rois = np.stack([np.zeros(n), x1, y1, x1 + r.uniform(8, 120, n), y1 + r.uniform(8, 100, n)], 1).astype(np.float32)
    feats = _features(n, 64, cuda, 3)
    for rows, k, thr in ((rois, 4, 300), (rois[:512], 9, 64)):
        res = {}
        for switch in ("0", "1"):
            monkeypatch.setenv("SCDA_DEVICE_KMEANS", switch)
            before = host_calls[0]
            np.random.seed(77)
            cf, centres = compute_cluster_targets(torch.from_numpy(rows), feats[:rows.shape[0]], N_cluster=k, threshold=thr)
            res[switch] = (cf, centres, np.random.get_state())
            assert host_calls[0] - before == 1
        assert torch.equal(res["1"][0], res["0"][0])
        # both are sklearn runs: its float32 centres repeat to ~1e-4 px only (tests/test_host_functions.py), hence the host path's bound
        np.testing.assert_allclose(res["1"][1], res["0"][1], rtol=0, atol=CENTRE_ATOL)
        np.testing.assert_array_equal(corners_of(res["1"][1]), corners_of(res["0"][1]))
        assert np.array_equal(res["1"][2][1], res["0"][2][1]) and res["1"][2][2] == res["0"][2][2]


def test_trainer_step_with_the_switch_on_equals_off(cuda, monkeypatch, host_calls):
    """one 256 x 512 iteration of ScdaTrainer from the same seeded weights, inputs and generators: the cluster features and the crop
    boxes are equal, and then every logged loss is equal bit for bit (only the centres' last bits can differ, and they feed only int())"""
    import model_common as mc
    from scda_amd import train_step
    from scda_amd.dropin.models.faster_rcnn import faster_rcnn_adver_expansion_reweight_cluster as model
    from test_train_step_gpu import build_product
    real_cluster, real_corner = model.compute_cluster_targets, train_step.get_corner_from_center
    seen = {}

    def cluster(*a, **kw):
        cf, centres = real_cluster(*a, **kw)
        seen["features"].append(cf)
        return cf, centres

    def corner(*a, **kw):
        boxes = real_corner(*a, **kw)
        seen["boxes"].append(boxes)
        return boxes

    monkeypatch.setattr(model, "compute_cluster_targets", cluster)
    monkeypatch.setattr(train_step, "get_corner_from_center", corner)
    res = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("SCDA_DEVICE_KMEANS", switch)
        seen.update(features=[], boxes=[])
        before = host_calls[0]
        torch.manual_seed(1)
        tr = train_step.ScdaTrainer(mc.CFG, cuda, lr=1e-3, new_w=512, new_h=256, models=mc.seeded_models(build_product))
        src, tgt, gts, info = mc.seeded_inputs(256, 512)
        np.random.seed(5)
        out = tr.step(src.to(cuda), gts, info, tgt.to(cuda))
        torch.cuda.synchronize()
        assert host_calls[0] - before == (0 if switch == "1" else 2)     # two calls per step; none goes back to the host with the switch on
        losses = {key: float(v) for key, v in out.items() if torch.is_tensor(v) and v.numel() == 1 or isinstance(v, float)}
        res[switch] = dict(features=[f.cpu() for f in seen["features"]], boxes=list(seen["boxes"]), losses=losses,
                           rng=(torch.rand(1).item(), np.random.rand()))
    assert len(res["0"]["features"]) == 2 and len(res["0"]["boxes"]) == 2 and len(res["0"]["losses"]) >= 8
    for a, b in zip(res["1"]["features"], res["0"]["features"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert res["1"]["boxes"] == res["0"]["boxes"]
    assert res["1"]["losses"] == res["0"]["losses"]
    assert res["1"]["rng"] == res["0"]["rng"]
