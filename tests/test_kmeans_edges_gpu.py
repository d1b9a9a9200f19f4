"""The k-means and cluster-gather kernels (scda_amd/csrc/cluster_ops.hip) on the MI355X at their edges: the cases of
tests/kmeans_edge_cases.py -- N at and around a wave (63 / 64 / 65, 127 / 128 / 129) and the cap (1023 / 1024), N = 1, N = k, k = 1,
exact distance ties, coincident points, a zero variance, duplicates -- against tests/kmeans_np.py bit for bit and against
scikit-learn's recorded answer (tests/golden/kmeans_edges_ref.npz, see tests/test_kmeans_edges_rules.py).  Every output lies in an
arena between sentinel words, so a write outside a buffer shows; the member lists are checked for their structure alone; the
outputs depend neither on what the buffers held nor on the launch before.  The gather at F = 1 .. 1028, on misaligned views, with
threshold = 1, threshold > N and broken member rows, against index_select bit for bit.  A NaN or infinite RoI coordinate raises
sklearn's ValueError with the switch on as with it off."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import kmeans_np as KN
import kmeans_edge_cases as EC
from test_kmeans_edges_rules import BY_NAME, CASES, CENTRE_ATOL, FALLBACK, check_against_sklearn, statement

pytestmark = pytest.mark.gpu

GUARD = 64                       # sentinel words before, between and after the buffers
SENTINEL = 0x5EA7BEEF
ORDER = ("centres", "labels", "counts", "members", "seed_index", "n_iter", "status")
CLASSES = sorted(set(c["cls"] for c in CASES))
_RUNS = {}


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


def seeding(n, k):
    from scda_amd import device_clusters
    if 1 <= k <= KN.MAX_K:
        return device_clusters.seeding_constants(n, k)[:2]
    return 0, (ctypes.c_double * ((k - 1) * 4))()         # beyond the rule: the kernel must refuse before it reads a draw


def arena_run(rois_np, k, dev, fill=-7):
    """scda_kmeans_hip with all seven outputs carved from ONE int32 arena, GUARD sentinel words before, between and after them, the
    outputs pre-filled with `fill` -> the outputs as numpy arrays.  Asserts that every sentinel is intact after the launch."""
    from scda_amd import native
    n = rois_np.shape[0]
    sizes = {"centres": 2 * k, "labels": n, "counts": k, "members": k * n, "seed_index": k, "n_iter": 1, "status": 1}
    arena = torch.full((GUARD + sum(sizes[key] + GUARD for key in ORDER),), SENTINEL, dtype=torch.int32, device=dev)
    bufs, spans, at = {}, {}, GUARD
    for key in ORDER:
        spans[key] = (at, at + sizes[key])
        bufs[key] = arena[at:at + sizes[key]]
        bufs[key].fill_(fill)
        at += sizes[key] + GUARD
    bufs["centres"] = bufs["centres"].view(torch.float32)
    rois = torch.from_numpy(np.ascontiguousarray(rois_np, dtype=np.float32)).to(dev)
    first, uniforms = seeding(n, k)
    native.kmeans(rois, k, first, uniforms, bufs)
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    inside = np.zeros(host.shape[0], dtype=bool)
    for a, b in spans.values():
        inside[a:b] = True
    assert int((~inside).sum()) == GUARD * (len(ORDER) + 1)
    hit = np.nonzero(~inside & (host != SENTINEL))[0]
    assert hit.size == 0, "sentinel words overwritten at %s (buffers at %s)" % (hit[:8].tolist(), spans)
    out = {key: host[a:b].copy() for key, (a, b) in spans.items()}
    out["centres"] = out["centres"].view(np.float32).reshape(k, 2)
    out["members"] = out["members"].reshape(k, n)
    return out


def kernel(c, dev):
    """the kernel's outputs on a case of the fixture, launched once and shared (read-only) by the tests below"""
    if c["name"] not in _RUNS:
        _RUNS[c["name"]] = arena_run(c["rois"], c["k"], dev)
    return _RUNS[c["name"]]


def same_bytes(a, b, keys=ORDER):
    for key in keys:
        assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------------------------------------------ a. statement and sklearn
@pytest.mark.parametrize("cls", CLASSES)
def test_kernel_equals_statement_and_sklearn(cuda, cls):
    """every case, kept or not: status, seed indices, labels, counts and n_iter equal the numpy statement's, the centres bit for bit;
    the kept cases also equal sklearn's recorded run"""
    for c in (c for c in CASES if c["cls"] == cls):
        out, km = kernel(c, cuda), statement(c)
        assert int(out["status"][0]) == km["status"] == 0, c["name"]
        np.testing.assert_array_equal(out["seed_index"], km["seed_index"], err_msg=c["name"])
        np.testing.assert_array_equal(out["labels"], km["labels"], err_msg=c["name"])
        np.testing.assert_array_equal(out["counts"], km["counts"], err_msg=c["name"])
        assert int(out["n_iter"][0]) == km["n_iter"], c["name"]
        np.testing.assert_array_equal(out["centres"].view(np.uint32), km["centres"].view(np.uint32), err_msg=c["name"])
        if c["equal"]:
            check_against_sklearn(dict(out, status=out["status"][0], n_iter=out["n_iter"][0]), c)
            np.testing.assert_array_equal(out["counts"], np.bincount(c["labels"], minlength=c["k"]), err_msg=c["name"])


# ------------------------------------------------------------------------------------------------ b. / c. buffers and structure
@pytest.mark.parametrize("cls", CLASSES)
def test_member_lists_partition_the_points(cuda, cls):
    """independent of both statements: the member lists are ascending and disjoint, their union is 0..N-1, counts sum to N, the
    tail of every row is -1 and labels[members[c, j]] == c.  (arena_run has checked the sentinels around every buffer.)"""
    for c in (c for c in CASES if c["cls"] == cls):
        out = kernel(c, cuda)
        n, k = c["rois"].shape[0], c["k"]
        counts, members, labels = out["counts"], out["members"], out["labels"]
        assert (counts >= 1).all() and int(counts.sum()) == n, c["name"]
        assert ((labels >= 0) & (labels < k)).all(), c["name"]
        seen = np.zeros(n, dtype=np.int32)
        for j in range(k):
            row = members[j, :counts[j]]
            assert (members[j, counts[j]:] == -1).all(), c["name"]
            assert ((row >= 0) & (row < n)).all() and (np.diff(row) > 0).all(), c["name"]
            assert (labels[row] == j).all(), c["name"]
            seen[row] += 1
        assert (seen == 1).all(), c["name"]
        assert 1 <= int(out["n_iter"][0]) <= KN.MAX_ITER and ((out["seed_index"] >= 0) & (out["seed_index"] < n)).all()


@pytest.mark.parametrize("c", FALLBACK, ids=[c["name"] for c in FALLBACK])
def test_fallback_cases_raise_bit_0_inside_the_buffers(cuda, c):
    """fewer than k distinct points at N = 2, 65 and 1024: status bit 0 as the statement says, nothing written outside the buffers;
    a run that ended DURING Lloyd (n_iter = 0) wrote counts = 0 and left labels and members alone"""
    out = arena_run(c["rois"], c["k"], cuda)
    assert int(out["status"][0]) == KN.kmeans(c["rois"], c["k"])["status"] == 1
    if int(out["n_iter"][0]) == 0:
        assert (out["counts"] == 0).all() and (out["labels"] == -7).all() and (out["members"] == -7).all()
    else:
        assert (out["counts"] == 0).any() and int(out["counts"].sum()) == c["rois"].shape[0]


def test_status_2_writes_status_and_n_iter_only(cuda):
    """N = 1025, k > N and k = 9: labels, members and every other output keep their pre-fill, the sentinels stay"""
    rois = EC.uniform(1, KN.CAPACITY + 1)
    for r, k in ((rois, 4), (rois, 8), (rois[:3], 4), (rois[:1], 2), (rois[:64], 9)):
        out = arena_run(r, k, cuda)
        assert int(out["status"][0]) == 2 and int(out["n_iter"][0]) == 0, (r.shape[0], k)
        assert KN.kmeans(r, k)["status"] == 2
        for key in ("labels", "members", "counts", "seed_index"):
            assert (out[key] == -7).all(), key
        assert (out["centres"].view(np.int32) == -7).all()


# ------------------------------------------------------------------------------------------------ d. no dependence on the past
@pytest.mark.parametrize("cls", CLASSES)
def test_outputs_do_not_depend_on_what_the_buffers_held(cuda, cls):
    for c in (c for c in CASES if c["cls"] == cls):
        same_bytes(arena_run(c["rois"], c["k"], cuda, fill=0x7fffffff), kernel(c, cuda))


def test_outputs_do_not_depend_on_the_launch_before(cuda):
    """(5, 2) after (1024, 8) -- whose points, labels and sums still lie in LDS -- gives the bytes of (5, 2) before it; and two runs of
    (1024, 8) and of (1, 1) are bit-identical"""
    small, big, one = BY_NAME["wave_5_2_s0"], BY_NAME["wave_1024_8_s0"], BY_NAME["wave_1_1_s0"]
    alone = arena_run(small["rois"], 2, cuda)
    first = arena_run(big["rois"], 8, cuda)
    after = arena_run(small["rois"], 2, cuda)
    same_bytes(after, alone)
    np.testing.assert_array_equal(after["centres"].view(np.uint32), statement(small)["centres"].view(np.uint32))
    same_bytes(arena_run(big["rois"], 8, cuda), first)
    a = arena_run(one["rois"], 1, cuda)
    same_bytes(arena_run(big["rois"], 8, cuda), first)
    same_bytes(arena_run(one["rois"], 1, cuda), a)
    assert a["labels"].tolist() == [0] and a["members"].tolist() == [[0]] and a["counts"].tolist() == [1]
    np.testing.assert_array_equal(a["centres"], KN.roi_centres(one["rois"]))


# ------------------------------------------------------------------------------------------------ e. row stride
def test_seven_column_rows(cuda):
    c = BY_NAME["wave_65_8_s0"]
    wide = np.concatenate([c["rois"], np.full((65, 2), 1e6, dtype=np.float32)], axis=1)
    assert wide.shape == (65, 7)
    same_bytes(arena_run(wide, 8, cuda), kernel(c, cuda))


# ------------------------------------------------------------------------------------------------ f. gather
def guarded_gather(src, members, counts, picks, k, thr, lead=GUARD):
    """native.cluster_gather through out= into a sentinel-guarded arena (`lead` words before the output: 64 keeps it 16-byte
    aligned, 65 does not) -> out [k, thr, F]; asserts the sentinels"""
    from scda_amd import native
    F = src.shape[1]
    size = k * thr * F
    arena = torch.full((lead + size + GUARD,), SENTINEL, dtype=torch.int32, device=src.device)
    out = arena[lead:lead + size].view(torch.float32).view(k, thr, F)
    got = native.cluster_gather(src, members, counts, picks, k, thr, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((arena[:lead] == SENTINEL).all()) and bool((arena[lead + size:] == SENTINEL).all()), "the gather wrote outside its output"
    return out


def gather_and_compare(src, members_np, counts_np, picks_np, thr, lead=GUARD):
    """members_np int32 [k, n], counts_np [k], picks_np int32 [k, thr] or None: the kernel against index_select on the rows the rule
    of include/scda_ops.h names (zeros where it names none), bit for bit"""
    dev = src.device
    k, n = members_np.shape
    F = src.shape[1]
    rows = np.full((k, thr), -1, dtype=np.int64)
    for c in range(k):
        for j in range(thr):
            if counts_np[c] >= thr:
                rows[c, j] = members_np[c, j] if j < n else -1
            elif picks_np is not None and 0 <= picks_np[c, j] < min(counts_np[c], n):
                rows[c, j] = members_np[c, picks_np[c, j]]
    ok = (rows >= 0) & (rows < n)
    want = src.index_select(0, torch.from_numpy(np.where(ok, rows, 0).reshape(-1)).to(dev)).view(k, thr, F).clone()
    want[torch.from_numpy(~ok).to(dev)] = 0.0
    got = guarded_gather(src, torch.from_numpy(members_np).to(dev), torch.from_numpy(counts_np.astype(np.int32)).to(dev),
                         None if picks_np is None else torch.from_numpy(picks_np).to(dev), k, thr, lead)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    return got, ok


def member_table(labels, k):
    n = labels.shape[0]
    members = np.full((k, n), -1, dtype=np.int32)
    counts = np.bincount(labels, minlength=k).astype(np.int32)
    for c in range(k):
        members[c, :counts[c]] = np.where(labels == c)[0]
    return members, counts


def features(n, F, dev, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((n, F)).astype(np.float32)).to(dev)


@pytest.mark.parametrize("F", [1, 3, 4, 5, 1024, 1028])
def test_gather_widths(cuda, F):
    """F = 1028 is 257 float4 per row: the vector loop's second trip, one lane wide; F = 1, 3, 5 take the scalar kernel; with every
    cluster longer than threshold (8) and every cluster shorter (48, picks)"""
    r = np.random.RandomState(F)
    n, k = 70, 2
    src = features(n, F, cuda, F)
    members, counts = member_table(r.randint(0, k, n), k)
    assert counts.min() >= 8 and counts.max() < 48
    gather_and_compare(src, members, counts, None, 8)
    gather_and_compare(src, members, counts, np.stack([r.randint(0, counts[c], 48) for c in range(k)]).astype(np.int32), 48)
    gather_and_compare(src, members, counts, None, 8, lead=GUARD + 1)         # an output that is not 16-byte aligned


@pytest.mark.parametrize("F", [8, 1028])
def test_gather_misaligned_views_take_the_scalar_kernel(cuda, F):
    """F % 4 == 0 rows that start 4 bytes into a 16-byte aligned row, and rows whose stride is no multiple of 4: float4 accesses would
    be misaligned, so the 4-byte kernel must answer -- with the same values"""
    r = np.random.RandomState(F + 1)
    n, k, thr = 33, 2, 4
    members, counts = member_table(r.randint(0, k, n), k)
    shifted = features(n, F + 8, cuda, 1)[:, 1:F + 1]
    odd_stride = features(n, F + 5, cuda, 2)[:, :F]
    aligned = features(n, F + 8, cuda, 3)[:, :F]
    assert shifted.data_ptr() % 16 == 4 and shifted.stride(0) % 4 == 0
    assert odd_stride.data_ptr() % 16 == 0 and odd_stride.stride(0) % 4 != 0
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(0) % 4 == 0 and aligned.stride(0) != F
    for src in (shifted, odd_stride, aligned):
        gather_and_compare(src, members, counts, None, thr)
        gather_and_compare(src, members, counts, np.stack([r.randint(0, counts[c], 40) for c in range(k)]).astype(np.int32), 40)


def test_gather_threshold_1_and_k_1(cuda):
    r = np.random.RandomState(7)
    n = 9
    src = features(n, 12, cuda, 7)
    for k in (1, 4):
        members, counts = member_table(np.arange(n) % k, k)
        got, ok = gather_and_compare(src, members, counts, None, 1)
        assert ok.all() and got.shape == (k, 1, 12)
        assert torch.equal(got[:, 0], src[:k])                                # the first member of cluster c is row c
    members, counts = member_table(np.zeros(n, dtype=np.int64), 1)            # k = 1: with and without picks
    gather_and_compare(src, members, counts, None, n)
    gather_and_compare(src, members, counts, r.randint(0, n, (1, 20)).astype(np.int32), 20)


def test_gather_threshold_above_n_and_n_1(cuda):
    r = np.random.RandomState(8)
    src = features(5, 4, cuda, 8)
    members, counts = member_table(np.array([0, 1, 0, 0, 1]), 2)
    picks = np.stack([r.randint(0, counts[c], 9) for c in range(2)]).astype(np.int32)
    got, ok = gather_and_compare(src, members, counts, picks, 9)
    assert ok.all()
    got, ok = gather_and_compare(src, members, counts, None, 9)               # no picks for short clusters: zeros
    assert not ok.any() and float(got.abs().max()) == 0.0
    for F in (1, 4):                                                          # N = 1
        one = features(1, F, cuda, 9)
        members, counts = member_table(np.zeros(1, dtype=np.int64), 1)
        got, ok = gather_and_compare(one, members, counts, None, 1)
        assert ok.all() and torch.equal(got.view(1, F), one)
        got, ok = gather_and_compare(one, members, counts, np.zeros((1, 4), dtype=np.int32), 4)
        assert ok.all() and torch.equal(got.view(4, F), one.expand(4, F))


def test_gather_counts_at_the_threshold_and_broken_rows(cuda):
    """clusters of exactly threshold, threshold - 1 and 0 members; a pick at count (one past the list) and a negative one; a -1
    inside the first threshold slots of a row whose count says it is long enough: rows of zeros, nothing read outside the table"""
    r = np.random.RandomState(9)
    thr, F = 6, 8
    labels = r.permutation(np.array([0] * thr + [1] * (thr - 1)))
    src = features(labels.shape[0], F, cuda, 10)
    members, counts = member_table(labels, 3)
    assert counts.tolist() == [thr, thr - 1, 0]
    picks = np.stack([r.randint(0, thr - 1, thr) for _ in range(3)]).astype(np.int32)
    got, ok = gather_and_compare(src, members, counts, picks, thr)
    assert ok[0].all() and ok[1].all() and not ok[2].any()
    picks[1, 2], picks[1, 4] = thr - 1, -1
    got, ok = gather_and_compare(src, members, counts, picks, thr)
    assert ok[1].tolist() == [True, True, False, True, False, True] and float(got[1, 2].abs().max()) == 0.0
    broken = members.copy()
    broken[0, 3] = -1
    got, ok = gather_and_compare(src, broken, counts, picks, thr)
    assert ok[0].tolist() == [True, True, True, False, True, True] and float(got[0, 3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ g. compute_cluster_targets
def both_switches(monkeypatch, host_calls, rois_np, feats, k, thr, seed, raises=None):
    """compute_cluster_targets with SCDA_DEVICE_KMEANS = 0 and 1 on the same seeded global generator -> per switch (features, centres,
    generator state, host-path calls), or with `raises` (the message the ValueError must carry) the last two"""
    from scda_amd import device_clusters
    from scda_amd.dropin.functions.mask import compute_cluster_targets
    res = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("SCDA_DEVICE_KMEANS", switch)
        assert device_clusters.enabled() == (switch == "1")
        before = host_calls[0]
        np.random.seed(seed)
        cf = centres = None
        if raises is None:
            cf, centres = compute_cluster_targets(torch.from_numpy(rois_np).to(feats.device), feats, N_cluster=k, threshold=thr)
            torch.cuda.synchronize()
        else:
            with warnings.catch_warnings(), pytest.raises(ValueError, match=raises):
                warnings.simplefilter("ignore")
                compute_cluster_targets(torch.from_numpy(rois_np).to(feats.device), feats, N_cluster=k, threshold=thr)
        res[switch] = (cf, centres, np.random.get_state(), host_calls[0] - before)
    assert np.array_equal(res["1"][2][1], res["0"][2][1]) and res["1"][2][2] == res["0"][2][2]      # the global generator
    return res


@pytest.mark.parametrize("name,thr", [("wave_1024_8_s0", 64), ("wave_1_1_s0", 1), ("n_eq_k_8", 128), ("wave_65_4_s0", 1), ("lattice_8x8_4", 16)])
def test_switch_on_equals_switch_off_at_the_edges(cuda, monkeypatch, host_calls, name, thr):
    from test_kmeans_rules import corners_of
    c = BY_NAME[name]
    n, k = c["rois"].shape[0], c["k"]
    assert c["equal"]
    feats = features(n, 32, cuda, n + k)
    feats[:, 0] = torch.arange(n, dtype=torch.float32, device=cuda)          # column 0 spells out the selected rows
    res = both_switches(monkeypatch, host_calls, c["rois"], feats, k, thr, 4321)
    assert res["0"][3] == 1 and res["1"][3] == 0                              # the device path itself, not its way back to the host
    on, off = res["1"], res["0"]
    assert on[0].shape == (k, thr, 32) and on[0].is_cuda and on[0].dtype == torch.float32 and not on[0].requires_grad
    assert torch.equal(on[0].view(torch.int32), off[0].view(torch.int32))
    rows = on[0][:, :, 0].cpu().numpy().astype(np.int64)
    assert (c["labels"][rows] == np.arange(k)[:, None]).all()                 # every selected row is a member of its cluster
    assert on[1].dtype == np.float32 and on[1].shape == (k, 2)
    np.testing.assert_allclose(on[1], off[1], rtol=0, atol=CENTRE_ATOL)
    np.testing.assert_array_equal(corners_of(on[1]), corners_of(off[1]))


# ------------------------------------------------------------------------------------------------ the non-finite coordinate
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("bad,message", [(np.nan, "contains NaN"), (np.inf, "contains infinity")], ids=["nan", "inf"])
def test_non_finite_coordinate_raises_as_the_host_path_does(cuda, monkeypatch, host_calls, k, bad, message):
    """one NaN or infinite RoI coordinate: the kernel raises status bit 2 before the seeding (as the statement does) and writes counts,
    n_iter and status only; compute_cluster_targets then raises sklearn's ValueError with the switch on as with it off, after one
    call of the host path, on the same state of the global generator.  (Before bit 2, k = 1 returned a NaN centre.)"""
    rois = EC.uniform(5, 65)
    rois[40, 3] = bad
    out = arena_run(rois, k, cuda)
    assert int(out["status"][0]) == KN.kmeans(rois, k)["status"] == 4
    assert int(out["n_iter"][0]) == 0 and (out["counts"] == 0).all()
    assert (out["labels"] == -7).all() and (out["members"] == -7).all() and (out["seed_index"] == -7).all()
    res = both_switches(monkeypatch, host_calls, rois, features(65, 16, cuda, 6), k, 8, 99, raises=message)
    assert res["0"][3] == 1 and res["1"][3] == 1
