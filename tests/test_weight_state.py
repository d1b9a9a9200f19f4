"""The host side of the weight state that lives between the modules and the convolution kernels (see weight_state_cases.py), without a
GPU: which counters a write moves, that native._pack_tag sees every one of them, that the folded weights of a frozen conv / BN pair
follow their five sources, and that broadcast_params sends everything state_dict() holds.  The device side is
tests/test_weight_state_gpu.py."""
import socket

import torch
import torch.multiprocessing as mp
import torch.nn as nn

import weight_state_cases as WS
from test_distributed_cpu import Tiny


def _net():
    return nn.ModuleDict({n: nn.Conv2d(ci, co, k, padding=p, bias=False) for n, (ci, co, k, p) in WS.LAYERS.items()})


def test_a_torch_write_into_the_bucket_moves_the_buckets_counter_only():
    """the facts _pack_tag rests on: after `p.data = view` the Parameter keeps a version counter of its own; flat.data, FlatAdam's
    bucket Parameter, a detached alias and a slice share ONE other counter; a collective moves neither"""
    from scda_amd.flat import FlatParams
    net = _net()
    flat = FlatParams(net)
    w = net["c32"].weight
    bucket = nn.Parameter(flat.data, requires_grad=True)          # as FlatAdam builds it
    alias, piece = flat.data.detach(), flat.data[4:8]
    for write in (lambda: flat.data.add_(1), lambda: bucket.mul_(2), lambda: alias.sub_(1), lambda: piece.zero_(),
                  lambda: flat.data.copy_(torch.ones_like(flat.data))):
        vp, vf = w._version, flat.data._version
        with torch.no_grad():
            write()
        assert w._version == vp and flat.data._version == vf + 1 == bucket._version == alias._version
    assert float(w.detach().sum()) == w.numel()                            # ... although the values of w did change
    vp, vf = w._version, flat.data._version
    with torch.no_grad():
        w.copy_(torch.zeros_like(w))
    assert w._version == vp + 1 and flat.data._version == vf
    assert float(flat.data[flat.offset[id(w)]:flat.offset[id(w)] + w.numel()].abs().sum()) == 0


def test_pack_tag_changes_with_every_kind_of_write():
    from scda_amd import native
    from scda_amd.flat import FlatParams
    net = _net()
    plain = nn.Conv2d(4, 4, 3).weight
    tags = [native._pack_tag(plain)]

    def moved(w):
        tags.append(native._pack_tag(w))
        assert tags[-1] != tags[-2], tags[-2:]
    with torch.no_grad():
        plain.mul_(2); moved(plain)
    plain.data.mul_(2)                                             # a raw write: no counter moves, its author bumps the epoch
    assert native._pack_tag(plain) == tags[-1]
    native.WEIGHT_EPOCH[0] += 1; moved(plain)
    flat = FlatParams(net)
    w = net["c32"].weight
    tags.append(native._pack_tag(w))
    assert native._pack_tag(plain) != native._pack_tag(w)
    with torch.no_grad():
        w.add_(1); moved(w)
        flat.data.add_(1); moved(w)
        flat.data[:4].zero_(); moved(w)                            # (a slice of the bucket that does not even hold w)
        net.load_state_dict({k: torch.zeros_like(v) for k, v in net.state_dict().items()}); moved(w)
    flat.epoch += 1; moved(w)
    native.WEIGHT_EPOCH[0] += 1                                    # the fallback epoch is not a bucket weight's business
    assert native._pack_tag(w) == tags[-1]
    assert native._pack_tag(net["p1x1"].weight)[-1] == tuple(net["p1x1"].weight.shape)


def _pair(which):
    from scda_amd import layers as L
    pair = nn.Sequential(L.Conv2d(WS.FOLD_C, WS.FOLD_C, kernel_size=3, padding=1, bias=False), L.BatchNorm2d(WS.FOLD_C, eps=0.0))
    pair.load_state_dict(WS.fold_state(which), strict=False)
    pair.eval()
    for p in pair.parameters():
        p.requires_grad_(False)
    return pair


def _fold_is_current(pair, what):
    from scda_amd.dropin.models.mask_rcnn.resnet import _frozen, folded_params
    assert _frozen(pair[0], pair[1])
    w, b = folded_params(pair[0], pair[1])
    state = {k: v.detach().cpu().clone() for k, v in pair.state_dict().items()}
    rw, rb = WS.fold_ref_params(state)
    assert torch.equal(w.cpu().double(), rw) and torch.equal(b.cpu().double(), rb), "%s: the folded weights are not those of the pair" % what
    return w


def test_folded_pair_follows_its_five_sources():
    """folded_params after each write against the fold of the pair's CURRENT state in fp64 (exact: weight_state_cases.FOLD_VAR);
    every write changes every folded element, so a fold served from before the write fails"""
    pair = _pair(0)
    new = WS.fold_state(1)
    first = _fold_is_current(pair, "first fold")
    assert _fold_is_current(pair, "second call") is first                   # cached: the same tensor
    with torch.no_grad():
        pair[0].weight.copy_(new["0.weight"]); _fold_is_current(pair, "conv.weight.copy_")
        pair[1].running_var.copy_(new["1.running_var"]); _fold_is_current(pair, "bn.running_var.copy_")
        pair[1].weight.copy_(new["1.weight"]); _fold_is_current(pair, "bn.weight.copy_")
        pair[1].running_mean.copy_(new["1.running_mean"]); _fold_is_current(pair, "bn.running_mean.copy_")
        pair[1].bias.copy_(new["1.bias"]); _fold_is_current(pair, "bn.bias.copy_")
    pair.load_state_dict(WS.fold_state(0), strict=False); _fold_is_current(pair, "load_state_dict")


def test_folded_pair_notices_buffers_that_module_to_replaced():
    """Module.to() / .double() / .cpu() put NEW tensors in place of the buffers, and a new tensor's version starts at 0: written while
    they were away (here: in float64), the BN statistics come back under the versions the fold was made from"""
    pair = _pair(0)
    pair[1].double().float()                                       # fresh buffers: every version at 0, as after module.to(device)
    assert pair[1].running_var._version == 0 and pair[1].running_mean._version == 0
    _fold_is_current(pair, "first fold")
    new = WS.fold_state(1)
    pair[1].double()
    with torch.no_grad():
        pair[1].running_var.copy_(new["1.running_var"]); pair[1].running_mean.copy_(new["1.running_mean"])
    pair[1].float()
    assert pair[1].running_var._version == 0 and pair[1].running_mean._version == 0
    _fold_is_current(pair, "BN buffers replaced by Module.float()")


# ---------------------------------------------------------------- two ranks
class TinyFrozen(Tiny):
    """test_distributed_cpu.Tiny plus what a detector has and Tiny lacks: parameters with requires_grad = False (a frozen stem, frozen BN
    affines), which FlatParams leaves outside the bucket"""
    def __init__(self):
        super().__init__()
        self.frozen = nn.Linear(2, 2)
        for p in self.frozen.parameters():
            p.requires_grad_(False)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import os
    for k in ("SLURM_PROCID", "SLURM_NTASKS", "SLURM_NODELIST"):
        os.environ.pop(k, None)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1")
    import torch.distributed as dist
    from scda_amd import native
    from scda_amd.dropin.utils.distributed_utils import broadcast_params, dist_init
    from scda_amd.flat import FlatParams
    dist_init(str(port), backend="gloo")
    torch.manual_seed(100 + rank)
    m = TinyFrozen()
    m.bn.running_mean.fill_(float(rank + 1))
    flat = FlatParams(m)
    assert not flat._inside(m.frozen.weight, flat.data)
    before = (flat.epoch, native.WEIGHT_EPOCH[0], flat.data._version, m.frozen.weight._version)
    broadcast_params(m)
    # a collective moves no version counter: broadcast_params itself tells the pack cache that the weights are new, those in the
    # bucket (flat.epoch) and those outside it (native.WEIGHT_EPOCH)
    assert (flat.data._version, m.frozen.weight._version) == before[2:]
    tags_moved = flat.epoch != before[0] and native.WEIGHT_EPOCH[0] != before[1]
    # a frozen conv / BN pair beside a trainable layer, as the stem and layer1 of the ResNet detector: folded on this rank's own values
    # (rank 1 holds the other value set) before the broadcast arrives
    from scda_amd.dropin.models.mask_rcnn.resnet import folded_params
    det = nn.ModuleDict({"head": nn.Linear(2, 2), "pair": _pair(rank)})
    FlatParams(det)
    warm = [t.clone() for t in folded_params(det["pair"][0], det["pair"][1])]
    versions = [t._version for t in det["pair"].state_dict().values()]
    broadcast_params(det)
    assert [t._version for t in det["pair"].state_dict().values()] == versions          # nothing a version-keyed cache could see
    fold = {"warm": warm, "after": [t.clone() for t in folded_params(det["pair"][0], det["pair"][1])],
            "state": {k: v.clone() for k, v in det["pair"].state_dict().items()}}
    torch.save({"state": {k: v.clone() for k, v in m.state_dict().items()}, "tags_moved": tags_moved, "fold": fold,
                "views": all(flat._inside(p, flat.data) for p in m.parameters() if p.requires_grad)}, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_broadcast_params_sends_frozen_parameters_and_reaches_warm_folds(tmp_path):
    """every state_dict() entry of a flattened module is rank 0's afterwards, as with the reference's broadcast of
    state_dict().values(): the bucket in one collective, and buffers AND frozen parameters beside it; a frozen conv / BN pair that
    was folded before the broadcast (resnet.folded_params: the only consumer of the detector's frozen stem) is folded again"""
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2))
    torch.manual_seed(100)
    want = TinyFrozen()
    want.bn.running_mean.fill_(1.0)
    assert list(r0["state"]) == list(r1["state"]) == list(want.state_dict()) and "frozen.weight" in r0["state"]
    for k, v in want.state_dict().items():
        assert torch.equal(r0["state"][k], v), "rank 0 changed its own %s" % k
        assert torch.equal(r1["state"][k], v), "rank 1 did not receive %s" % k
    assert r0["views"] and r1["views"]
    assert r0["tags_moved"] and r1["tags_moved"], "broadcast_params left the packed-weight caches of the old weights valid"
    # the frozen pair: each rank's fold was warm on its own values; afterwards both hold rank 0's state AND its fold
    for r, res, own in ((0, r0, 0), (1, r1, 1)):
        f = res["fold"]
        for got, ref in zip(f["warm"], WS.fold_ref_params(WS.fold_state(own))):
            assert torch.equal(got.double(), ref), "rank %d: first fold" % r
        for k, v in WS.fold_state(0).items():
            assert torch.equal(f["state"][k], v), "rank %d did not receive the pair's %s" % (r, k)
        for got, ref in zip(f["after"], WS.fold_ref_params(WS.fold_state(0))):
            assert torch.equal(got.double(), ref), "rank %d: the fold of a frozen pair is still that of the weights from before the broadcast" % r
