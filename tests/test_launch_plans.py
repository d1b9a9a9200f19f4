"""The launch decision of every convolution / dense GEMM shape the workload and the GPU tests use, pinned on the CPU.
csrc/launch_plan.h decides kernel family, tile, split-K count, tile order and grid with host arithmetic only;
scda_debug_plan_conv / scda_debug_plan_gemm (native.plan_conv / plan_gemm) return that decision without a GPU, for a 256-CU
device.  tests/golden/launch_plans.json holds the table (tests/golden/make_golden_launch_plans.py writes it from `cases()`):
a kernel or planner change that moves a decision shows up here as a diff of named shapes, before any GPU run.
The stride-1 3x3 layers of at least 32 channels do not run those plans: route_conv sends them to the Winograd kernels, whose
decisions (decide_wino / decide_wino_wgrad through native.plan_wino) and routes tests/golden/wino_plans.json pins the same way."""
import json
import os

import pytest

from conftest import ROOT
import test_conv_wino_gpu as wn
import test_gemm_x9_gpu as x9
import test_tile_instantiations_gpu as ti

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
WINO_GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_plans.json")

# the layers of scripts/tune_plans.py (its module runs on import): (name, batch, Cin, H, W, Cout, k, stride, pad, row_period)
VGG = [(n, b, ci, h, w, co, 3, 1, 1, 0) for n, b, ci, h, w, co in (
    ("conv1_2", 1, 64, 512, 1024, 64), ("conv2_1", 1, 64, 256, 512, 128), ("conv2_2", 1, 128, 256, 512, 128),
    ("conv3_1", 1, 128, 128, 256, 256), ("conv3_2", 1, 256, 128, 256, 256), ("conv4_1", 1, 256, 64, 128, 512),
    ("conv4_2", 1, 512, 64, 128, 512), ("conv5_x", 1, 512, 32, 64, 512), ("dec_res", 4, 128, 64, 64, 128),
    ("dec_up1", 4, 128, 128, 128, 64), ("dec_up2", 4, 64, 256, 256, 32))]
RESNET = [("l2_c1", 1, 512, 100, 168, 128, 1, 1, 0, 0), ("l2_c2", 1, 128, 100, 168, 128, 3, 1, 1, 0), ("l2_c3", 1, 128, 100, 168, 512, 1, 1, 0, 0),
          ("l3_c1", 1, 1024, 50, 84, 256, 1, 1, 0, 0), ("l3_c2", 1, 256, 50, 84, 256, 3, 1, 1, 0), ("l3_c3", 1, 256, 50, 84, 1024, 1, 1, 0, 0),
          ("rpn", 1, 1024, 50, 84, 512, 3, 1, 1, 0),
          ("h_c1a", 1, 1024, 3584, 7, 512, 1, 1, 0, 0), ("h_c2", 1, 512, 3584, 7, 512, 3, 1, 1, 7), ("h_c3", 1, 512, 3584, 7, 2048, 1, 1, 0, 0),
          ("h_c1b", 1, 2048, 3584, 7, 512, 1, 1, 0, 0), ("h_ds", 1, 1024, 3584, 7, 2048, 1, 1, 0, 0)]


def _linear(kind, M, N, K):
    """plan_gemm arguments of native.linear_fwd / linear_dgrad / linear_wgrad for x [M][K], w [N][K]"""
    if kind == "fwd":
        return (M, N, K, K, K, False, False)
    if kind == "dgrad":
        return (M, K, N, N, K, False, True)
    return (N, K, M, N, K, True, True)


def cases():
    """[(key, "conv" | "gemm", arguments, environment)] -- the key names the case in the golden file"""
    out, keys = [], set()

    def conv(tag, direction, shape, rp=0, env=None):
        key = "%s %s %s rp%d%s" % (tag, direction, "x".join(map(str, shape)), rp, "".join(" %s=%s" % kv for kv in sorted((env or {}).items())))
        if key not in keys:      # (the tests' lists re-target some plans onto the same call)
            keys.add(key)
            out.append((key, "conv", (direction,) + tuple(shape) + (rp,), env or {}))

    def gemm(tag, args, env=None):
        key = "%s gemm %s%s" % (tag, "x".join(str(int(a)) for a in args), "".join(" %s=%s" % kv for kv in sorted((env or {}).items())))
        if key not in keys:
            keys.add(key)
            out.append((key, "gemm", tuple(args), env or {}))

    def forced(plan, bm64=False):
        env = {"SCDA_PLAN_FORCE": "%d,%d,%d" % tuple(plan)}
        if bm64:
            env["SCDA_PLAN_ALLOW_BM64"] = "1"
        return env

    # the workload's layers: forward, data gradient, weight gradient
    for layer in VGG + RESNET:
        for direction in ("fwd", "dgrad", "wgrad"):
            conv(layer[0], direction, layer[1:9], layer[9])
    # tests/test_tile_instantiations_gpu.py: every shape unforced ...
    conv_shapes = []
    for shape in [c for c, _ in ti.FWD_DGRAD] + [c for c, _ in ti.TILE32] + [c for c, _ in ti.WGRAD]:
        if shape not in conv_shapes:
            conv_shapes.append(shape)
    for shape in conv_shapes:
        for direction in ("fwd", "dgrad", "wgrad_bias"):
            conv("tile", direction, shape)
    fc_shapes = []
    for shape in [s for s, _ in ti.FC] + [s for s, _ in ti.FC_WGRAD]:
        if shape not in fc_shapes:
            fc_shapes.append(shape)
    for shape in fc_shapes:
        for kind in ("fwd", "dgrad", "wgrad"):
            gemm("fc_" + kind, _linear(kind, *shape))
    # ... and under the plans the tests force, legal and illegal, exactly as they force them
    for shape, plan in ti.FWD_DGRAD:
        conv("tile", "fwd", shape, env=forced(plan, plan[0] == 64 and shape[4] > 64))
        cin = shape[1]
        bm, bn, sp = plan
        natural = 64 if cin <= 64 else 128
        if not (bm == natural or (bm == 256 and cin % 256 == 0) or (bm == 64 and 64 < cin <= 128)):
            bm = natural
        if bn == 256 and bm != 64:
            bn = 128
        conv("tile", "dgrad", shape, env=forced((bm, bn, sp), bm == 64 and cin > 64))
    for shape, direction in ti.TILE32:
        conv("tile", direction, shape, env=forced((32, 256, 1)))
    for shape, plan in ti.WGRAD:
        conv("tile", "wgrad_bias", shape, env=forced(plan))
    for shape, plan in ti.FC:
        gemm("fc_fwd", _linear("fwd", *shape), forced(plan))
        gemm("fc_dgrad", _linear("dgrad", *shape), forced(plan))
    for shape, plan in ti.FC_WGRAD:
        gemm("fc_wgrad", _linear("wgrad", *shape), forced(plan))
    conv("tile", "fwd", ti.CONV1_2, env=forced((256, 128, 1)))      # test_illegal_force_is_ignored_and_visible
    for plan in ((256, 128, 1), (128, 128, 1), (64, 64, 300), (32, 128, 2)):      # illegal for a 32-row layer / too many splits
        conv("tile", "fwd", ti.TILE32[0][0], env=forced(plan))
        conv("tile", "wgrad_bias", ti.TILE32[0][0], env=forced(plan))
    # tests/test_gemm_x9_gpu.py: the FC6 / FC7-sized products and the small ones, by default and with the kernel forced / kept out
    for M, N, K, ta, tb in x9.CASES + [(1024, 1152, 512, True, True), (512, 2944, 1024, False, True)]:
        for env in ({}, {"SCDA_GEMM_X9": "2"}, {"SCDA_GEMM_X9": "0"}, {"SCDA_GEMM_X9": "2", "SCDA_GEMM_X9_SK": "2"}, {"SCDA_GEMM_X9": "2", "SCDA_GEMM_X9_SK": "0"}):
            gemm("x9", (M, N, K, M if ta else K, N if tb else K, ta, tb), env)
    for kind in ("fwd", "dgrad", "wgrad"):
        gemm("fc7_" + kind, _linear(kind, 512, 4096, 4096))
        gemm("fc6_" + kind, _linear(kind, 512, 4096, 25088))
        gemm("head_" + kind, _linear(kind, 512, 36, 4096))
    for (M, N, K, ta, tb), splits in (((512, 384, 2048, False, False), 4), ((260, 132, 1024, False, True), 3), ((300, 256, 1040, True, True), 2)):
        gemm("x9", (M, N, K, M if ta else K, N if tb else K, ta, tb), {"SCDA_GEMM_X9": "2", "SCDA_GEMM_X9_SPLITS": str(splits)})
    for cin, cout, h, w in ((512, 1024, 448, 7), (1024, 512, 448, 7), (256, 1024, 50, 84), (2048, 512, 112, 7)):      # batch-1 1x1 -> x9 routing
        for direction in ("fwd", "dgrad", "wgrad"):
            conv("x9", direction, (1, cin, h, w, cout, 1, 1, 0), env={"SCDA_GEMM_X9": "2"})
    return out


def wino_cases():
    """[(key, "wino" | "route", arguments, environment)]: plan_wino(kind, batch, Cin, H, W, Cout, row_period) of the layers as the
    forward convolution has them, and the route (family, pool, maps) of (direction, batch, Cin, H, W, Cout, k, stride, pad, row_period)"""
    out, keys = [], set()

    def add(kind, key, args, env):
        key += "".join(" %s=%s" % kv for kv in sorted((env or {}).items()))
        if key not in keys:
            keys.add(key)
            out.append((key, kind, tuple(args), env or {}))

    def wino(tag, kind, shape, rp=0, env=None):
        add("wino", "%s %s %s rp%d" % (tag, kind, "x".join(map(str, shape)), rp), (kind,) + tuple(shape) + (rp,), env)

    def route(tag, direction, shape, rp=0, env=None):
        add("route", "%s route %s %s rp%d" % (tag, direction, "x".join(map(str, shape)), rp), (direction,) + tuple(shape) + (rp,), env)

    def stacked(case):
        R, cin, cout = case
        return (1, cin, R * 7, 7, cout)

    # the workload's 3x3 layers: the route of every direction, and the Winograd decisions where it leads there
    for name, b, ci, h, w, co, k, s, p, rp in VGG + RESNET:
        for direction in ("fwd", "dgrad", "wgrad"):
            route(name, direction, (b, ci, h, w, co, k, s, p), rp)
        if k != 3:
            continue
        for kind in ("fwd", "dgrad", "dgrad_mask", "wgrad", "wgrad_bias"):
            wino(name, kind, (b, ci, h, w, co), rp)
        if decide("route", ("fwd", b, ci, h, w, co, k, s, p, rp), {})[1]:
            wino(name, "fwd_pool", (b, ci, h, w, co), rp)
    # tests/test_conv_wino_gpu.py: every shape unforced ...
    for shape in wn.WINO_CASES + [c for c, _ in wn.GM_CASES] + wn.PERSIST_CASES + [c for c, _ in wn.FORCED_SPLIT_CASES]:
        for kind in ("fwd",) + (("dgrad", "dgrad_mask") if shape[4] % 8 == 0 else ()):
            wino("wino", kind, shape)
    for shape in wn.WGRAD_CASES + [c for c, _ in wn.WGRAD_SPLIT_CASES]:
        for kind in ("wgrad", "wgrad_bias"):
            wino("wino", kind, shape)
    for case in wn.STACKED_CASES:
        for kind in ("fwd", "dgrad", "dgrad_mask"):
            wino("stack", kind, stacked(case), 7)
    for case in wn.STACKED_WGRAD_CASES:
        wino("stack", "wgrad_bias", stacked(case), 7)
    # ... and under the variables that file forces, exactly as it forces them
    for shape, gm in wn.GM_CASES:
        for v in (0, gm):
            wino("wino", "fwd", shape, env={"SCDA_WINO_GM": str(v)})
    for shape, splits in wn.WGRAD_SPLIT_CASES:
        wino("wino", "wgrad_bias", shape, env={"SCDA_WINO_WGRAD_SPLITS": str(splits), "SCDA_WINO_WGRAD_NO_GROUPS": "1"})
        wino("wino", "wgrad_bias", shape, env={"SCDA_WINO_WGRAD_SPLITS": str(splits)})
    for shape in wn.PERSIST_CASES:
        for mode in ("1", "0"):
            for kind in ("fwd", "dgrad_mask") + (("fwd_pool",) if shape[2] % 4 == 0 and shape[3] % 4 == 0 else ()):
                wino("wino", kind, shape, env={"SCDA_WINO_PERSIST": mode})
    for shape, splits in wn.FORCED_SPLIT_CASES:
        wino("wino", "fwd", shape, env={"SCDA_WINO_SPLITS": str(splits)})
    for case in wn.STACKED_CASES + wn.STACKED_WGRAD_CASES:
        for direction in ("fwd", "dgrad", "wgrad"):
            for env in ({}, {"SCDA_WINO_STACKED": "0"}):
                route("stack", direction, stacked(case) + (3, 1, 1), 7, env)
    return out


PLAN_ENV = ("SCDA_PLAN_FORCE", "SCDA_PLAN_ALLOW_BM64", "SCDA_PLAN_OVERRIDE", "SCDA_PLAN_LOG", "SCDA_GEMM_X9", "SCDA_GEMM_X9_SK", "SCDA_GEMM_X9_SPLITS",
            "SCDA_WINOGRAD", "SCDA_WINO_STACKED", "SCDA_CONV_POOL_FUSE", "SCDA_WINO_GM", "SCDA_WINO_SPLITS", "SCDA_WINO_PERSIST",
            "SCDA_WINO_WGRAD_SPLITS", "SCDA_WINO_WGRAD_NO_GROUPS", "SCDA_WINO_DBG", "SCDA_WINO_LOG")


def decide(kind, args, env):
    from scda_amd import native
    saved = {k: os.environ.pop(k, None) for k in PLAN_ENV}
    os.environ.update(env)
    try:
        if kind == "wino":
            return list(native.plan_wino(*args).values())
        if kind == "route":
            return [int(v) for v in native._route(("fwd", "dgrad", "wgrad").index(args[0]), *args[1:6], args[6], *args[6:])]
        d = native.plan_conv(*args) if kind == "conv" else native.plan_gemm(*args)
    finally:
        for k in PLAN_ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return [d[f] for f in native.PLAN_FIELDS]


def test_launch_plans_match_the_table():
    golden = json.load(open(GOLDEN))
    from scda_amd import native
    assert golden["fields"] == list(native.PLAN_FIELDS)
    got = {key: decide(kind, args, env) for key, kind, args, env in cases()}
    assert sorted(got) == sorted(golden["plans"]), "the case list and the table differ: regenerate only with a reason"
    wrong = {k: (dict(zip(native.PLAN_FIELDS, golden["plans"][k])), dict(zip(native.PLAN_FIELDS, v))) for k, v in got.items() if v != golden["plans"][k]}
    assert not wrong, "launch decisions moved (table, now):\n" + "\n".join("%s\n  %s\n  %s" % (k, a, b) for k, (a, b) in wrong.items())


def test_every_kernel_family_and_tile_is_in_the_table():
    """the table is not vacuous: all four families, the stream-K and split-K x9 forms, parity classes, both weight-gradient slab
    depths and every tile shape of the instantiation lists occur"""
    plans = [dict(zip(json.load(open(GOLDEN))["fields"], v)) for v in json.load(open(GOLDEN))["plans"].values()]
    assert {p["family"] for p in plans} == {0, 1, 2}      # (3, the small-Cin direct forward, is pinned below: no such layer in the lists)
    assert {(p["bm"], p["bn"]) for p in plans if p["family"] == 1} >= {(32, 256), (32, 128), (64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (256, 128)}
    assert any(p["x9_stream"] for p in plans) and any(p["family"] == 2 and p["splits"] > 1 for p in plans)
    assert any(p["parity"] for p in plans) and any(p["swz"] == 3 for p in plans)
    assert {p["wbk"] for p in plans if p["family"] == 0 and p["wbk"]} == {16, 32}


def test_wino_plans_and_routes_match_the_table():
    golden = json.load(open(WINO_GOLDEN))
    from scda_amd import native
    assert golden["fields"] == list(native.WINO_PLAN_FIELDS) and golden["wgrad_fields"] == list(native.WINO_WGRAD_PLAN_FIELDS)
    got = {key: decide(kind, args, env) for key, kind, args, env in wino_cases()}
    assert sorted(got) == sorted(golden["plans"]), "the case list and the table differ: regenerate only with a reason"
    wrong = {k: (golden["plans"][k], v) for k, v in got.items() if v != golden["plans"][k]}
    assert not wrong, "Winograd decisions / routes moved (table, now):\n" + "\n".join("%s\n  %s\n  %s" % (k, a, b) for k, (a, b) in wrong.items())


def test_every_winograd_launch_form_is_in_the_table():
    """the Winograd table is not vacuous: both tile-row values, both XCD orders, every gm, a split launch, both persistent states, all
    four epilogues, the three weight-gradient orders, a stacked launch and all three routes occur"""
    from scda_amd import native
    golden = json.load(open(WINO_GOLDEN))
    kind = lambda key: key.split()[1]
    fwd = [dict(zip(golden["fields"], v)) for k, v in golden["plans"].items() if kind(k) in ("fwd", "fwd_pool", "dgrad", "dgrad_mask")]
    wgrad = [dict(zip(golden["wgrad_fields"], v)) for k, v in golden["plans"].items() if kind(k) in ("wgrad", "wgrad_bias")]
    routes = {k: v for k, v in golden["plans"].items() if kind(k) == "route"}
    assert len(fwd) + len(wgrad) + len(routes) == len(golden["plans"])
    assert {p["mb"] for p in fwd} == {1, 2} and {p["pixel_major"] for p in fwd} == {0, 1} and {p["gm"] for p in fwd} == {1, 2, 4}
    assert any(p["splits"] > 1 for p in fwd) and {p["persist"] for p in fwd} == {0, 1} and {p["epi"] for p in fwd} == {0, 1, 2, 3}
    assert {p["order"] for p in wgrad} == {0, 1, 2} and any(p["splits"] > 1 and p["order"] == 0 for p in wgrad)
    assert {v[0] for v in routes.values()} == {0, 1, 2} and any(v[1] for v in routes.values())
    assert any(" rp7" in k and kind(k) == "fwd" for k in golden["plans"]) and any(" rp7" in k and kind(k) == "wgrad_bias" for k in golden["plans"])


def test_winograd_routing_on_the_cpu(monkeypatch):
    """what tests/test_conv_wino_gpu.py asserts about the routes, without a device: the 32-channel floor on either side, stride, row
    period, even maps, the stacks of 7 x 7 maps and their switch, the data gradient's swapped channels, the pool threshold"""
    from scda_amd import native
    for v in PLAN_ENV:
        monkeypatch.delenv(v, raising=False)
    assert not native.wino_ok(1, 16, 32, 64, 64, 3, 3, 1, 1) and not native.wino_ok(1, 64, 32, 64, 16, 3, 3, 1, 1)
    assert not native.wino_ok(1, 128, 32, 64, 128, 3, 3, 2, 1)
    assert not native.wino_ok(1, 128, 32, 64, 128, 3, 3, 1, 1, row_period=8)
    assert native.wino_ok(1, 128, 30, 64, 128, 3, 3, 1, 1) and not native.wino_ok(1, 128, 31, 64, 128, 3, 3, 1, 1)      # any EVEN height / width
    assert not native.wino_wgrad_ok(1, 16, 32, 64, 64, 3, 3, 1, 1) and not native.wino_wgrad_ok(1, 64, 32, 64, 64, 3, 3, 2, 1)
    assert native.wino_wgrad_ok(1, 32, 32, 64, 64, 3, 3, 1, 1) and native.wino_wgrad_ok(1, 64, 32, 64, 32, 3, 3, 1, 1)     # from 32 channels a side
    assert native.wino_wgrad_ok(1, 64, 32, 72, 64, 3, 3, 1, 1) and not native.wino_wgrad_ok(1, 64, 32, 71, 64, 3, 3, 1, 1)
    for R, Cin, Cout in wn.STACKED_CASES:
        assert native.wino_ok(1, Cin, R * 7, 7, Cout, 3, 3, 1, 1, 7) and native.wino_stacked(1, R * 7, 7, 7) == R
    for R, Cin, Cout in wn.STACKED_WGRAD_CASES:
        assert native.wino_wgrad_ok(1, Cin, R * 7, 7, Cout, 3, 3, 1, 1, 7)
    assert not native.wino_wgrad_ok(1, 72, 37 * 7, 7, 40, 3, 3, 1, 1, 7)           # the stacked weight gradient needs 64 channels a side
    # the data gradient reduces over Cout: Cout % 8 decides, Cin need not be a multiple of 8
    assert native._route(1, 1, 36, 32, 64, 64, 3, 3, 1, 1, 0)[0] == 1 and native._route(0, 1, 36, 32, 64, 64, 3, 3, 1, 1, 0)[0] == 0
    assert native._route(1, 1, 64, 32, 64, 36, 3, 3, 1, 1, 0)[0] == 0 and native._route(0, 1, 64, 32, 64, 36, 3, 3, 1, 1, 0)[0] == 1
    # conv + pool: from 200 64-row tiles (here 1 x 25 x 8 against 1 x 25 x 7 blocks of 8 x 32 pixels), never on stacked maps
    assert native.conv_pool_fusable(1, 64, 200, 256, 64, 3, 3, 1, 1) and not native.conv_pool_fusable(1, 64, 200, 224, 64, 3, 3, 1, 1)
    assert native.conv_pool_fusable(1, 64, 200, 224, 128, 3, 3, 1, 1) and not native.conv_pool_fusable(1, 64, 512 * 7, 7, 64, 3, 3, 1, 1, 7)
    monkeypatch.setenv("SCDA_CONV_POOL_FUSE", "0")
    assert not native.conv_pool_fusable(1, 64, 200, 256, 64, 3, 3, 1, 1) and native.wino_ok(1, 64, 200, 256, 64, 3, 3, 1, 1)
    monkeypatch.setenv("SCDA_WINO_STACKED", "0")
    for R, Cin, Cout in wn.STACKED_CASES:
        assert not native.wino_ok(1, Cin, R * 7, 7, Cout, 3, 3, 1, 1, 7)
    for R, Cin, Cout in wn.STACKED_WGRAD_CASES:
        assert not native.wino_wgrad_ok(1, Cin, R * 7, 7, Cout, 3, 3, 1, 1, 7)
    monkeypatch.setenv("SCDA_WINOGRAD", "0")
    assert not native.wino_enabled() and not native.wino_ok(1, 128, 32, 64, 128, 3, 3, 1, 1) and not native.wino_wgrad_ok(1, 128, 32, 64, 128, 3, 3, 1, 1)


def test_input_conditions_select_the_families():
    """what the retired switches used to force is reached from the input alone"""
    from scda_amd import native
    fam = lambda *a, **k: native.plan_conv(*a, **k)["family"]
    assert fam("fwd", 1, 3, 64, 128, 64, 3, 1, 1) == 3                       # image-side 3x3: the direct kernel
    assert fam("fwd", 1, 3, 64, 32, 64, 3, 1, 1) == 0                        # ... narrower than 64 pixels: register-staged gather
    assert fam("fwd", 1, 24, 32, 32, 64, 3, 1, 1) == 0 and fam("fwd", 1, 32, 32, 32, 64, 3, 1, 1) == 1      # Cin % 16
    assert fam("wgrad", 1, 64, 50, 84, 64, 3, 1, 1) == 0 and fam("wgrad", 1, 64, 48, 84, 64, 3, 1, 1) == 1  # OH*OW % 16
    assert fam("wgrad", 1, 64, 48, 84, 64, 3, 1, 1, aligned=False) == 0
    assert native.plan_gemm(512, 1024, 512, 512, 512)["family"] == 1 and native.plan_gemm(512, 1024, 512, 512, 512, aligned=False)["family"] == 0
    assert native.plan_gemm(512, 1024, 520, 520, 520)["family"] == 0         # K % 16
    d = native.plan_conv("dgrad", 4, 32, 32, 32, 64, 3, 2, 1)
    assert d["parity"] == 1 and native.plan_conv("dgrad", 4, 32, 31, 31, 64, 3, 2, 1)["parity"] == 0       # odd planes: no parity classes


@pytest.mark.parametrize("override,want", [("64,2048,1152:64,64,1", (64, 64, 1)), ("64,2048,1152:256,128,1", None), ("1,2,3:64,64,1", None)])
def test_plan_override_uses_the_same_legality_test(override, want):
    """SCDA_PLAN_OVERRIDE names one shape "M,N,K:bm,bn,splits": taken when legal for that shape, ignored otherwise"""
    shape = ("fwd", 1, 128, 32, 64, 64, 3, 1, 1, 0)      # M = 64, N = 2048, K = 1152
    base = decide("conv", shape, {})
    got = decide("conv", shape, {"SCDA_PLAN_OVERRIDE": override})
    assert tuple(got[2:5]) == (want or tuple(base[2:5]))
