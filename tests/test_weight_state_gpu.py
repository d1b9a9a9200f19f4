"""The state between the modules and the convolution kernels, on the device: native._PACK_CACHE, native.conv2d_pack_all, the re-homing
of parameters into a FlatParams bucket and the folded weights of a frozen conv / BN pair, against EVERY way the weights are written
(weight_state_cases.py; the host-side facts are pinned by tests/test_weight_state.py).

Every case warms the derived copies with a forward + backward, writes the weights, and runs forward + backward again.  Then
  * the reference is the fp64 convolution of tests/conv_refs.py with the weights the module holds NOW (read back after the write):
    rule B of tests/test_conv_edges_gpu.py (integer operands, 4 max S < 2^24 asserted, torch.equal) for every writer that can write
    integers -- they write 3 - w, so a stale copy is wrong everywhere -- and rule A as written there (check_rule_a, FACTOR, ULP4, the
    fp32 CPU evaluation) for the Adam step, which with lr = 0.5 moves every weight by about 0.5: a stale copy misses that bound by
    five orders of magnitude;
  * the same call on w.detach().clone() -- a plain tensor is never cached -- gives the same bits.  The uncached call is compared with
    the reference FIRST: a failure there is a kernel error, a difference between the two calls is a stale copy.
Every call proves the kernels it ran: native.lib() is wrapped (Calls) and records each launch entry point with the plan the library
reports right behind it, which must be launch_plan.h's decision for the route the case names; a route not taken fails."""
import os
import socket
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import conv_refs as R
import weight_state_cases as WS
from test_conv_edges_gpu import FACTOR, ULP4, bits, check_exact, check_rule_a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

PACKS = ("scda_conv2d_pack_weight_hip", "scda_conv2d_wino_pack_hip")
CONVS = ("scda_conv2d_wino_hip", "scda_conv2d_fwd_hip", "scda_conv2d_dgrad_act_hip")
BIG, ODD, P1X1 = ("c32", 8, 8, "wino"), ("c32", 7, 8, "gemm"), ("p1x1", 8, 8, "gemm")


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault(cuda):
    """a device fault is sticky: nothing more is launched behind one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault, stopping the run: %s" % e, returncode=3)


class Calls:
    """native.lib() with a record of every launch entry point (scda_*_hip) called through it: (name, native.last_plan(),
    native.wino_last_order()) read right behind the call"""
    def __init__(self, native, real):
        self._native, self._real, self.log = native, real, []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.endswith("_hip"):
            return f

        def call(*a):
            r = f(*a)
            self.log.append((name, self._native.last_plan(), self._native.wino_last_order()))
            return r
        return call

    def names(self):
        return [e[0] for e in self.log]

    def packs(self):
        return [n for n in self.names() if n in PACKS]


@pytest.fixture
def env(cuda, monkeypatch):
    from scda_amd import native
    monkeypatch.delenv("SCDA_WINOGRAD", raising=False)
    assert native.wino_enabled()
    rec = Calls(native, native.lib())
    monkeypatch.setattr(native, "lib", lambda: rec)
    return types.SimpleNamespace(native=native, calls=rec, dev=cuda)


# ---------------------------------------------------------------- one forward + backward, proved and compared
def fwd_bwd(w, call, x, dy, dev):
    from scda_amd import autograd_ops as A
    xg = x.to(dev).requires_grad_()
    y = A.conv2d(xg, w, None, 1, WS.LAYERS[call[0]][3])
    y.backward(dy.to(dev))
    return y.detach(), xg.grad


def assert_route(native, log, call):
    """the forward and the data gradient ran the kernels the case names, on launch_plan.h's plan for them"""
    name, H, W, route = call
    Cin, Cout, k, pad = WS.LAYERS[name]
    assert native.wino_ok(1, Cin, H, W, Cout, k, k, 1, pad) == (route == "wino"), call
    ran = [e for e in log if e[0] in CONVS]
    if route == "wino":
        assert [e[0] for e in ran] == ["scda_conv2d_wino_hip"] * 2, (call, [e[0] for e in log])
        for (_, _, order), kind in zip(ran, ("fwd", "dgrad")):
            plan = native.plan_wino(kind, 1, Cin, H, W, Cout)
            assert order[0] == (plan["mb"], bool(plan["pixel_major"]), plan["gm"], plan["splits"]), (call, kind, order, plan)
    else:
        assert [e[0] for e in ran] == ["scda_conv2d_fwd_hip", "scda_conv2d_dgrad_act_hip"], (call, [e[0] for e in log])
        for (_, lp, _), kind in zip(ran, ("fwd", "dgrad")):
            plan = native.plan_conv(kind, 1, Cin, H, W, Cout, k, 1, pad)
            assert lp[:3] == (plan["bm"], plan["bn"], plan["splits"]) and (lp[3] is True) == (plan["family"] == 1), (call, kind, lp, plan)


def check_now(env, w, call, what, seed=0, rule="B"):
    """forward + backward through the Parameter `w` as it is now -> the per-layer pack launches the call needed.  Rule "B": exact;
    rule "A": the componentwise bound of test_conv_edges_gpu (printed with pytest -s)"""
    x, dy = WS.int_operands(call, seed)
    label = "%s/%s-%dx%d-%s" % ((what,) + tuple(call))
    env.calls.log.clear()
    y, dx = fwd_bwd(w, call, x, dy, env.dev)
    log = list(env.calls.log)
    assert_route(env.native, log, call)
    env.calls.log.clear()
    y0, dx0 = fwd_bwd(w.detach().clone(), call, x, dy, env.dev)
    assert_route(env.native, env.calls.log, call)
    f_fwd, f_dgrad = WS.refs(call, w.detach().cpu(), x, dy)
    if rule == "B":
        check_exact(label + " uncached forward", y0, f_fwd)
        check_exact(label + " uncached data gradient", dx0, f_dgrad)
    else:
        Kf, Kd = WS.chain_terms(call)
        factor = FACTOR["wino" if call[3] == "wino" else "direct"]
        check_rule_a(label + " uncached forward", call[3], y0, f_fwd, Kf, factor)
        check_rule_a(label + " uncached data gradient", call[3], dx0, f_dgrad, Kd, factor)
    for got, base, which in ((y, y0, "forward"), (dx, dx0, "data gradient")):
        bad = int((bits(got) != bits(base)).sum())
        assert bad == 0, "%s: the %s through the pack cache differs from the uncached call on the same values in %d of %d elements: " \
                         "a stale copy was served" % (label, which, bad, got.numel())
    return [e[0] for e in log if e[0] in PACKS]


def assert_warm(env, w, call):
    for d in WS.LAYOUTS[call[3]]:
        hit = env.native._PACK_CACHE.get((w.data_ptr(), d))
        assert hit is not None and hit[2]() is w, (call, d)
    assert check_now(env, w, call, "warm, second call") == [], "a warm weight was packed again"


# ---------------------------------------------------------------- nets, buckets, writers
def make_net(dev, seed=0, flip=False, extra=()):
    """one Conv2d per WS.LAYERS entry (+ `extra`: (name, LAYERS key) pairs), integer weights"""
    from scda_amd import layers as L
    spec = [(n, n) for n in WS.LAYERS] + list(extra)
    net = nn.ModuleDict()
    for i, (name, key) in enumerate(spec):
        ci, co, k, p = WS.LAYERS[key]
        net[name] = L.Conv2d(ci, co, kernel_size=k, padding=p, bias=False)
        w = WS.int_weight(key, seed + i)
        with torch.no_grad():
            net[name].weight.copy_(WS.flipped(w) if flip else w)
    return net.to(dev)


def trainer_standin(net, dev, lr=0.5):
    """what checkpoint.save_checkpoint / restore touch of a ScdaTrainer (as tests/test_checkpoint.py builds it), around tiny nets"""
    from scda_amd import layers as L
    from scda_amd.flat import FlatAdam, FlatParams
    tr = types.SimpleNamespace(model=net, dec=L.Conv2d(4, 4, kernel_size=1).to(dev), dis=L.Conv2d(4, 4, kernel_size=1).to(dev),
                               dis_patch=L.Conv2d(4, 4, kernel_size=1).to(dev))
    tr.flat = {k: FlatParams(m) for k, m in (('det', tr.model), ('dec', tr.dec), ('dis', tr.dis), ('dis_patch', tr.dis_patch))}
    tr.opt = {k: FlatAdam(f, lr) for k, f in tr.flat.items()}
    return tr


def current(net):
    return {n: m.weight.detach().cpu().clone() for n, m in net.items()}


def write(env, kind, net, tr, tmp_path):
    """change every weight of `net` the way `kind` names -> (rule, the values the weights must hold now or None)"""
    from scda_amd import checkpoint as C
    new = {n: WS.flipped(v) for n, v in current(net).items()}
    if kind == "adam_step":
        tr.opt['det'].step()
        return "A", None
    with torch.no_grad():
        if kind == "param_copy":
            for n, m in net.items():
                m.weight.copy_(new[n].to(env.dev))
        elif kind == "load_state_dict":
            net.load_state_dict({n + ".weight": v for n, v in new.items()})
        elif kind == "bucket_copy":                      # a torch write into the bucket: what a collective does
            flat = net._scda_flat
            new_flat = flat.data.clone()
            for n, m in net.items():
                off = flat.offset[id(m.weight)]
                new_flat[off:off + m.weight.numel()] = new[n].reshape(-1).to(env.dev)
            flat.data.copy_(new_flat)
        elif kind == "checkpoint_restore":
            twin = trainer_standin(make_net(env.dev), env.dev)
            for n, m in twin.model.items():
                m.weight.copy_(new[n].to(env.dev))
            C.restore(tr, C.save_checkpoint(twin, str(tmp_path / "ck.pth"), epoch=1))
        elif kind == "raw_write_weight_epoch":           # no counter moves (.data has one of its own): the author bumps the epoch
            for n, m in net.items():
                v = m.weight._version
                m.weight.data.copy_(new[n].to(env.dev))
                assert m.weight._version == v
            env.native.WEIGHT_EPOCH[0] += 1
        else:
            raise KeyError(kind)
    return "B", new


def write_and_check(env, kind, net, tr, tmp_path, w, call):
    before = current(net)
    rule, new = write(env, kind, net, tr, tmp_path)
    name = next(n for n, m in net.items() if m.weight is w)
    now = current(net)
    if new is None:
        moved = (now[name] - before[name]).abs()
        assert float(moved.max()) > 0.25 and float((moved > 0.25).float().mean()) > 0.5, "the Adam step did not move the weights"
        # ... far enough: the convolution with the weights from before the step misses rule A's floor by more than three orders
        x, dy = WS.int_operands(call, 1)
        (y_new, S), (y_old, _) = WS.refs(call, now[name], x, dy)[0](torch.float64), WS.refs(call, before[name], x, dy)[0](torch.float64)
        assert float(((y_old - y_new).abs() / S.clamp_min(1.0)).max()) > 1e3 * ULP4
    else:
        assert all(torch.equal(now[n], new[n]) for n in new), "the writer did not write"
    return check_now(env, w, call, kind, seed=1, rule=rule)


@pytest.mark.parametrize("call", WS.CALLS, ids=WS.CALL_IDS)
@pytest.mark.parametrize("writer", WS.BUCKET_WRITERS)
def test_write_to_a_bucket_weight_reaches_all_four_layouts(env, tmp_path, writer, call):
    net = make_net(env.dev)
    tr = trainer_standin(net, env.dev)
    w = net[call[0]].weight
    assert w._scda_flat is tr.flat['det'] and tr.flat['det']._inside(w, tr.flat['det'].data)
    check_now(env, w, call, "warm")
    assert_warm(env, w, call)
    packs = write_and_check(env, writer, net, tr, tmp_path, w, call)
    if writer == "adam_step":
        assert packs == [], "conv2d_pack_all behind the step left a layout to the lazy path: %s" % packs
    else:
        assert len(packs) == 2, packs                    # forward and data-gradient layout, each packed once
    assert check_now(env, w, call, writer + ", second call", seed=2, rule="A" if writer == "adam_step" else "B") == []


@pytest.mark.parametrize("call", WS.CALLS, ids=WS.CALL_IDS)
@pytest.mark.parametrize("writer", WS.PLAIN_WRITERS)
def test_write_to_a_parameter_outside_every_bucket(env, tmp_path, writer, call):
    net = make_net(env.dev)
    w = net[call[0]].weight
    assert getattr(w, "_scda_flat", None) is None
    check_now(env, w, call, "warm")
    assert_warm(env, w, call)
    assert len(write_and_check(env, writer, net, None, tmp_path, w, call)) == 2
    assert check_now(env, w, call, writer + ", second call", seed=2) == []


@pytest.mark.parametrize("call", WS.CALLS, ids=WS.CALL_IDS)
def test_flattening_after_the_first_backward_rehomes_the_weight(env, tmp_path, call):
    """FlatParams(module, keep_grads=True) behind a forward + backward (the lazy flattening of average_gradients): the weight moves
    into the bucket, its copies are made again there and follow a write into the bucket; the entry left under the OLD address is not
    served to an unrelated weight that lands on it (the `hit[2]() is w` test of the cache).  That collision is SIMULATED where the
    allocator does not produce it: a same-sized Parameter is allocated after the old storage is gone, its version is brought to the
    one in the entries' tags, and if it did not get the old block the entries are copied under ITS address -- so the tag matches
    either way and only the identity test stands between the new weight and the old weight's copies."""
    from scda_amd.flat import FlatParams
    N = env.native
    net = make_net(env.dev)
    w = net[call[0]].weight
    old_ptr = w.data_ptr()
    check_now(env, w, call, "warm")
    assert_warm(env, w, call)
    old_values = w.detach().cpu().clone()
    assert w.grad is not None
    g = w.grad.detach().clone()
    flat = FlatParams(net, keep_grads=True)
    assert w.data_ptr() != old_ptr and flat._inside(w, flat.data) and torch.equal(w.grad, g) and torch.equal(w.detach().cpu(), old_values)
    assert len(check_now(env, w, call, "re-homed")) == 2
    assert len(write_and_check(env, "bucket_copy", net, None, tmp_path, w, call)) == 2
    left = {d: N._PACK_CACHE.get((old_ptr, d)) for d in WS.LAYOUTS[call[3]]}
    assert all(e is not None for e in left.values())
    other = nn.Parameter(WS.flipped(old_values).to(env.dev))         # same size: the allocator may hand it the freed block
    with torch.no_grad():
        while other._version < max(e[0][0] for e in left.values()):    # ... and everything else the entry's tag holds
            other.add_(0)
    if other.data_ptr() != old_ptr:       # it did not: put the entries where a weight that had taken the block would find them
        for d, e in left.items():
            N._PACK_CACHE[(other.data_ptr(), d)] = e
    assert len(check_now(env, other, call, "unrelated weight on the old address", seed=2)) == 2


# ---------------------------------------------------------------- plan flips of conv2d_pack_all
def plan_bucket(dev, names=("l0", "l1", "l2"), with_1x1=True, seed=0):
    from scda_amd import layers as L
    from scda_amd.flat import FlatAdam, FlatParams
    net = nn.ModuleDict()
    for i, n in enumerate(names):
        net[n] = L.Conv2d(32, 32, kernel_size=3, padding=1, bias=False)
        with torch.no_grad():
            net[n].weight.copy_(WS.int_weight("c32", seed + i))
    if with_1x1:
        net["p"] = L.Conv2d(32, 16, kernel_size=1, bias=False)
        with torch.no_grad():
            net["p"].weight.copy_(WS.int_weight("p1x1", seed))
    net.to(dev)
    flat = FlatParams(net)
    assert len(flat.conv_weights) == len(net)
    return net, flat, FlatAdam(flat, 0.5)


def layer_calls(net, flags):
    """(weight, the call that runs last) per layer: an eligible layer's flag is the route of its last forward"""
    out = [(net[n].weight, BIG if f else ODD) for n, f in zip([n for n in net if n != "p"], flags)]
    return out + ([(net["p"].weight, P1X1)] if "p" in net else [])


def pack_through_cache(native, w, d):
    return native.conv2d_pack_weight(w, d) if isinstance(d, bool) else native.conv2d_wino_pack(w, d == 3)


def fresh_pack(native, w, d):
    t = w.detach().clone()
    return native.conv2d_pack_weight(t, d, cache=False) if isinstance(d, bool) else native.conv2d_wino_pack(t, d == 3, cache=False)


def step_to(env, net, flat, opt, flags, rule):
    """leave every layer's route flag as `flags` says, step, and check everything the step left behind"""
    N = env.native
    opt.zero_grad()
    for w, call in layer_calls(net, flags):
        check_now(env, w, call, "before the step %s" % (flags,), rule=rule)
    assert tuple(bool(w._scda_wino_used) for w in flat.conv_weights[:len(flags)]) == tuple(flags)
    env.calls.log.clear()
    opt.step()
    # the step is its two launches: nothing packs per layer, nothing else was added to it
    assert env.calls.names() == ["scda_adam_limited_hip", "scda_conv2d_pack_weights_batched_hip"], env.calls.names()
    assert next(reversed(flat._scda_pack_plans)) == tuple(flags) + ((False,) if "p" in net else ())
    label = "behind the step %s" % (flags,)
    # 1. what the step seeded is served as it is -- no lazy pack -- and equals the per-layer pack of the weights as they are now
    for w, call in layer_calls(net, flags):
        for d in WS.LAYOUTS[call[3]]:
            env.calls.log.clear()
            got = pack_through_cache(N, w, d)
            assert env.calls.packs() == [], (label, call, d)
            want = fresh_pack(N, w, d)
            assert got.shape == want.shape and torch.equal(bits(got), bits(want)), (label, call, d)
            out = flat._scda_pack_out                       # ... and is the copy the step wrote into the bucket's one buffer
            assert out.data_ptr() <= got.data_ptr() and got.data_ptr() + got.numel() * 4 <= out.data_ptr() + out.numel() * 4
        assert check_now(env, w, call, label, seed=1, rule="A") == [], "a same-size forward behind the step packed lazily"
    # 2. the other route in the same epoch (the lazy path): right too, and packed once
    for w, call in layer_calls(net, flags)[:len(flags)]:
        other = ODD if call is BIG else BIG
        assert len(check_now(env, w, other, label + ", the other size", seed=2, rule="A")) == 2
        assert check_now(env, w, other, label + ", the other size again", seed=3, rule="A") == []
    # 3. everything the cache hands out for these weights now, seeded or lazy
    n = 0
    for w in flat.conv_weights:
        for d in (False, True, 2, 3):
            if (w.data_ptr(), d) in N._PACK_CACHE:
                got, want = pack_through_cache(N, w, d), fresh_pack(N, w, d)
                assert torch.equal(bits(got), bits(want)), (label, tuple(w.shape), d)
                n += 1
    assert n == 4 * len(flags) + (2 if "p" in net else 0), n


T, F = True, False


def test_pack_all_plan_flips_and_flips_back(env):
    """P1: all three layers on the Winograd kernels, one of them on an odd map for a step, then back"""
    net, flat, opt = plan_bucket(env.dev)
    for i, flags in enumerate([(T, T, T), (T, F, T), (T, T, T)]):
        step_to(env, net, flat, opt, flags, "B" if i == 0 else "A")
    assert len(flat._scda_pack_plans) == 2


def test_pack_all_more_plans_than_it_keeps_and_a_growing_buffer(env):
    """P2 + P3: six of the eight flag tuples and back to the first (four plans are kept), in an order in which the layouts' total --
    a Winograd layout is larger than a GEMM-ready one -- exceeds every earlier total three times: the ONE output buffer all plans
    share is replaced, and what is served before and after each replacement is right"""
    N = env.native
    net, flat, opt = plan_bucket(env.dev)
    walk = [(F, F, F), (T, F, F), (F, T, F), (T, T, F), (F, T, T), (T, T, T), (F, F, F)]
    elems = lambda d: int(N.lib().scda_conv2d_packed_elems(32, 32, 3, 3, d))
    assert elems(2) + elems(3) > elems(0) + elems(1)
    bufs, sizes = [], []
    for i, flags in enumerate(walk):
        if i == len(walk) - 1:
            assert len(flat._scda_pack_plans) == 4 and not any(k[:3] == walk[0] for k in flat._scda_pack_plans)     # (dropped by now)
        step_to(env, net, flat, opt, flags, "B" if i == 0 else "A")
        bufs.append(flat._scda_pack_out.data_ptr())
        sizes.append(flat._scda_pack_out.numel())
    assert len(flat._scda_pack_plans) == 4 and next(reversed(flat._scda_pack_plans))[:3] == walk[0]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4, sizes
    for i in range(1, len(walk)):         # a larger total: a new buffer (allocated while the old one is still held); else the same one
        assert (bufs[i] != bufs[i - 1]) == (sizes[i] > sizes[i - 1]), (i, sizes, bufs)


def test_two_buckets_stepped_alternately(env):
    """P4: a step on bucket A leaves the copies of B's weights valid, correct and THE SAME tensors; B's own step replaces them"""
    N = env.native
    a_net, a_flat, a_opt = plan_bucket(env.dev, names=("l0",), with_1x1=False, seed=0)
    b_net, b_flat, b_opt = plan_bucket(env.dev, names=("l0",), with_1x1=False, seed=5)
    step_to(env, a_net, a_flat, a_opt, (T,), "B")
    step_to(env, b_net, b_flat, b_opt, (T,), "B")
    wa, wb = a_net["l0"].weight, b_net["l0"].weight
    for call in (BIG, ODD):                                       # B's four layouts are warm in B's current epoch
        assert check_now(env, wb, call, "B warm", rule="A") == []
    entries = {d: N._PACK_CACHE[(wb.data_ptr(), d)] for d in (False, True, 2, 3)}
    step_to(env, a_net, a_flat, a_opt, (T,), "A")
    for d, e in entries.items():
        assert N._PACK_CACHE[(wb.data_ptr(), d)] is e and pack_through_cache(N, wb, d) is e[1], d
        assert torch.equal(bits(e[1]), bits(fresh_pack(N, wb, d))), d
    for call in (BIG, ODD):
        assert check_now(env, wb, call, "B behind A's step", seed=1, rule="A") == []
    step_to(env, b_net, b_flat, b_opt, (T,), "A")
    for d in (2, 3):
        assert N._PACK_CACHE[(wb.data_ptr(), d)] is not entries[d] and N._PACK_CACHE[(wb.data_ptr(), d)][0] != entries[d][0]
    for call in (BIG, ODD):
        check_now(env, wa, call, "A behind B's step", seed=2, rule="A")


# ---------------------------------------------------------------- folded frozen pairs
def make_pair(dev):
    from scda_amd import layers as L
    pair = nn.Sequential(L.Conv2d(WS.FOLD_C, WS.FOLD_C, kernel_size=3, padding=1, bias=False), L.BatchNorm2d(WS.FOLD_C, eps=0.0))
    pair.load_state_dict(WS.fold_state(0), strict=False)
    pair.eval()
    for p in pair.parameters():
        p.requires_grad_(False)
    return pair.to(dev)          # (new buffer tensors: their versions start at 0 on the device)


def fold_check(env, pair, what, seed=0):
    from scda_amd import autograd_ops as A
    from scda_amd.dropin.models.mask_rcnn.resnet import _frozen, folded_conv_bn
    assert _frozen(pair[0], pair[1]), what
    x = R.ints((1, WS.FOLD_C, WS.FOLD_HW, WS.FOLD_HW), -R.INT_X, R.INT_X, 5000 + seed)
    env.calls.log.clear()
    y = folded_conv_bn(x.to(env.dev), pair[0], pair[1], A.ACT_RELU)
    ran = [n for n in env.calls.names() if n in CONVS]
    assert ran == ["scda_conv2d_fwd_hip"] and not env.native.wino_ok(1, WS.FOLD_C, WS.FOLD_HW, WS.FOLD_HW, WS.FOLD_C, 3, 3, 1, 1), ran
    state = {k: v.detach().cpu().clone() for k, v in pair.state_dict().items()}
    w64, b64 = WS.fold_ref_params(state)
    S = torch.nn.functional.conv2d(x.double().abs(), w64.abs(), b64.abs(), padding=1)
    assert 4 * S.max().item() * 64 < 2 ** 24                   # every partial sum is a multiple of 2^-6 (weight_state_cases.FOLD_VAR)
    want = WS.fold_ref(state, x)
    # the same convolution on a fold made from scratch from the same state: a plain tensor pair that no cache knows
    w0, b0 = (t.float().to(env.dev) for t in (w64, b64))
    y0 = A.conv2d(x.to(env.dev), w0, b0, 1, 1, A.ACT_RELU, 0.0)
    assert torch.equal(y0.cpu().double(), want), "%s: kernel error on a fresh fold" % what
    bad = int((bits(y) != bits(y0)).sum())
    assert bad == 0, "%s: folded_conv_bn differs from the fold of the pair's current state in %d of %d elements: a stale fold was " \
                     "served" % (what, bad, y.numel())


def test_folded_pair_follows_every_write(env):
    pair = make_pair(env.dev)
    new = {k: v.to(env.dev) for k, v in WS.fold_state(1).items()}
    fold_check(env, pair, "first fold")
    first = pair[0]._scda_folded
    fold_check(env, pair, "second call", seed=1)
    assert pair[0]._scda_folded is first                          # cached
    with torch.no_grad():
        pair[0].weight.copy_(new["0.weight"]); fold_check(env, pair, "conv.weight.copy_", 2)
        pair[1].running_var.copy_(new["1.running_var"]); fold_check(env, pair, "bn.running_var.copy_", 3)
        pair[1].weight.copy_(new["1.weight"]); fold_check(env, pair, "bn.weight.copy_", 4)
    pair.load_state_dict(WS.fold_state(0), strict=False); fold_check(env, pair, "load_state_dict", 5)


def test_folded_pair_notices_bn_buffers_that_went_through_the_host(env):
    """bn.cpu() ... bn.to(device): the buffers come back as NEW tensors at version 0 -- the version the first fold saw on the device --
    and were written while on the host"""
    pair = make_pair(env.dev)
    assert pair[1].running_var._version == 0 and pair[1].running_mean._version == 0
    fold_check(env, pair, "first fold")
    new = WS.fold_state(1)
    pair[1].cpu()
    with torch.no_grad():
        pair[1].running_var.copy_(new["1.running_var"]); pair[1].running_mean.copy_(new["1.running_mean"])
    pair[1].to(env.dev)
    assert pair[1].running_var._version == 0 and pair[1].running_mean._version == 0
    fold_check(env, pair, "BN buffers back from the host", 1)


# ---------------------------------------------------------------- two ranks
RANK_CALLS = [(c[0], c) for c in WS.CALLS] + [("frozen", BIG), ("frozen", ODD)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_net(dev, flip):
    net = make_net(dev, flip=flip, extra=[("frozen", "c32")])
    net["frozen"].weight.requires_grad_(False)
    return net


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from scda_amd import native
    from scda_amd.dropin.utils.distributed_utils import broadcast_params
    from scda_amd.flat import FlatParams
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    net = _rank_net(dev, flip=rank == 1)
    flat = FlatParams(net)
    assert not flat._inside(net["frozen"].weight, flat.data)

    def run_all(seed):
        out = {}
        for name, call in RANK_CALLS:
            x, dy = WS.int_operands(call, seed)
            Cin, Cout, k, pad = WS.LAYERS[call[0]]          # (the route: the single-process tests prove kernel and plan for these shapes)
            assert native.wino_ok(1, Cin, call[1], call[2], Cout, k, k, 1, pad) == (call[3] == "wino"), call
            y, dx = fwd_bwd(net[name].weight, call, x, dy, dev)
            assert bool(getattr(net[name].weight, "_scda_wino_used", None)) == (call[3] == "wino"), call
            out["%s-%dx%d" % (name, call[1], call[2])] = (y.cpu(), dx.cpu())
        return out
    first = run_all(0)                       # every derived copy is warm, made from THIS rank's weights
    broadcast_params(net)
    second = run_all(1)
    torch.cuda.synchronize()
    torch.save({"first": first, "second": second, "state": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}},
               os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_broadcast_reaches_warm_caches_and_frozen_parameters(cuda, tmp_path):
    """validate, resume, broadcast: each rank has run a forward + backward on its own weights (rank 1's are 3 - w) when
    broadcast_params arrives.  Afterwards rank 1 computes what rank 0 computes -- the exact convolution with rank 0's weights, on all
    four layouts, the frozen layer included -- and every state_dict() entry is rank 0's"""
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2))
    want = {n + ".weight": m.weight.detach().clone() for n, m in _rank_net(torch.device("cpu"), flip=False).items()}
    assert list(r0["state"]) == list(r1["state"]) == list(want)
    for k, v in want.items():
        assert torch.equal(r0["state"][k], v), "rank 0 changed its own %s" % k
        assert torch.equal(r1["state"][k], v), "rank 1 did not receive %s" % k
    for name, call in RANK_CALLS:
        key = "%s-%dx%d" % (name, call[1], call[2])
        assert not torch.equal(r0["first"][key][0], r1["first"][key][0]), key          # the caches were warmed on different weights
        x, dy = WS.int_operands(call, 1)
        f_fwd, f_dgrad = WS.refs(call, want[name + ".weight"], x, dy)
        for r, res in ((0, r0), (1, r1)):
            check_exact("rank %d %s forward behind the broadcast" % (r, key), res["second"][key][0], f_fwd)
            check_exact("rank %d %s data gradient behind the broadcast" % (r, key), res["second"][key][1], f_dgrad)
        assert torch.equal(bits(r0["second"][key][0]), bits(r1["second"][key][0])) and torch.equal(bits(r0["second"][key][1]), bits(r1["second"][key][1]))
