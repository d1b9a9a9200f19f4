"""Training the keypoint branch on the device: the heat-map loss kernels (scda_amd/csrc/keypoint_loss.hip) against float64 on the CPU at
their edge shapes and layouts, the head + loss against torch's own layers, the stacked channel-major branch against the [R, C, 14, 14]
batch in training mode (with the loss path's padding of the RoI list), and full SCDA iterations with the keypoint loss."""
import numpy as np
import pytest
import torch

from gpu_arrays import words
from test_resnet_oracle_gpu import CFG as RCFG, rel_l2

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard words on each side of an output buffer
SENTINEL = 0x5a5a5a5a


def guarded(shape, cuda):
    """-> (the whole buffer as int32, a contiguous float32 view of `shape` in its middle)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=cuda)
    return buf, buf[GUARD:GUARD + n].view(torch.float32).view(shape)


def guards_intact(buf):
    w = words(buf)
    return bool((w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all())


def ref64(heat, targets):
    """float64 on the CPU: (mean over the counted pairs of -log_softmax(map)[target], count, d loss / d heat)"""
    R, Kp, h, w = heat.shape
    x = heat.double().reshape(R * Kp, h * w).requires_grad_()
    t = targets.reshape(-1).long()
    on = t >= 0
    n = int(on.sum())
    if n == 0:
        return 0.0, 0, torch.zeros(R, Kp, h, w, dtype=torch.float64)
    loss = -torch.log_softmax(x[on], dim=1).gather(1, t[on][:, None]).sum() / n
    loss.backward()
    return float(loss.detach()), n, x.grad.reshape(R, Kp, h, w)


def run_kernels(cuda, heat, targets, transposed):
    """the two entry points on guarded buffers, twice -> (out2 [2], gradient [R, Kp, h, w]) on the host; asserts that the second
    launch gives the same bits and that no guard word changed"""
    from scda_amd import native as N
    R, Kp, h, w = heat.shape
    if transposed:                                                 # the values through the keypoint head's [Kp, R, h, w] view
        x = heat.transpose(0, 1).contiguous().to(cuda).transpose(0, 1)
        assert not x.is_contiguous() or R == 1 or Kp == 1
    else:
        x = heat.to(cuda)
    t = targets.to(cuda)
    g = torch.tensor([0.75], device=cuda)
    runs = []
    for _ in range(2):
        sbuf, stats = guarded((R * Kp, 2), cuda)
        lbuf, row_loss = guarded((R * Kp,), cuda)
        dbuf, d = guarded((Kp, R, h, w) if transposed else (R, Kp, h, w), cuda)
        d = d.transpose(0, 1) if transposed else d
        out2, _, _ = N.keypoint_ce_fwd(x, t, stats=stats, row_loss=row_loss)
        got = N.keypoint_ce_bwd(x, t, stats, out2, g, out=d)
        torch.cuda.synchronize()
        assert got.data_ptr() == d.data_ptr() and guards_intact(sbuf) and guards_intact(lbuf) and guards_intact(dbuf)
        assert SENTINEL not in words(stats.contiguous()) and SENTINEL not in words(row_loss)      # fully written
        runs.append((out2.cpu(), got.cpu().contiguous(), stats.cpu(), row_loss.cpu()))
    for a, b in zip(*runs):
        assert np.array_equal(words(a), words(b)), "two launches on the same input differ"
    return runs[0][0], runs[0][1] / 0.75


def check(cuda, heat, targets, transposed=False):
    out2, grad = run_kernels(cuda, heat, targets, transposed)
    want, n, want_grad = ref64(heat, targets)
    print("keypoint loss %s%s: loss %.8g (fp64 %.8g), count %d, gradient rel l2 %.2e"
          % (tuple(heat.shape), " transposed" if transposed else "", float(out2[0]), want, n, rel_l2(grad, want_grad) if n else 0.0))
    assert float(out2[1]) == n
    assert bool(torch.isfinite(out2).all()) and bool(torch.isfinite(grad).all())
    assert abs(float(out2[0]) - want) <= 1e-5 * abs(want)
    off = (targets < 0)
    assert not grad[off].any() and np.all(words(grad[off]) == 0)             # exactly +0.0 on uncounted maps
    if n:
        assert rel_l2(grad, want_grad) <= 1e-4
    else:
        assert float(out2[0]) == 0.0 and not grad.any()
    return out2, grad


def seeded(shape, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    R, Kp, h, w = shape
    heat = torch.randn(shape, generator=g) * scale
    targets = torch.randint(0, h * w, (R, Kp), generator=g, dtype=torch.int32)
    return heat, targets


def test_56x56_contiguous_and_transposed(cuda):
    heat, targets = seeded((3, 2, 56, 56), 1)
    targets[1, 0] = -1
    a2, ag = check(cuda, heat, targets)
    b2, bg = check(cuda, heat, targets, transposed=True)
    assert abs(float(a2[0]) - float(b2[0])) <= 1e-6 * abs(float(a2[0])) and float(a2[1]) == float(b2[1]) == 5
    assert rel_l2(bg, ag) <= 1e-6


@pytest.mark.parametrize("shape", [(2, 1, 1, 1), (2, 3, 7, 9), (1, 1, 64, 64)], ids=["HW1", "HW63_below_a_wave", "HW4096_the_cap"])
def test_edge_sizes(cuda, shape):
    heat, targets = seeded(shape, 2)
    out2, grad = check(cuda, heat, targets)
    check(cuda, heat, targets, transposed=True)
    if shape[2] * shape[3] == 1:
        assert float(out2[0]) == 0.0 and not grad.any()


def test_counted_sets_at_the_configured_map_count(cuda):
    """(5, 17, 56, 56): no counted pair, exactly one, and the first and last position as targets"""
    heat, _ = seeded((5, 17, 56, 56), 3)
    none = torch.full((5, 17), -1, dtype=torch.int32)
    out2, grad = check(cuda, heat, none, transposed=True)
    assert out2.tolist() == [0.0, 0.0] and not grad.any()
    one = none.clone()
    one[3, 11] = 1234
    out2, grad = check(cuda, heat, one, transposed=True)
    assert float(out2[1]) == 1.0 and grad[3, 11].any()
    ends = none.clone()
    ends[0, 0], ends[4, 16], ends[2, 5], ends[2, 6] = 0, 56 * 56 - 1, 56 * 56 - 1, 0
    check(cuda, heat, ends)
    check(cuda, heat, ends, transposed=True)


def test_large_logits_stay_finite(cuda):
    heat, targets = seeded((2, 2, 56, 56), 4, scale=1.0)
    heat[0, 0, 3, 3], heat[0, 0, 40, 7] = 1.0e4, -1.0e4
    heat[1, 1, 0, 0], heat[1, 1, 55, 55] = -1.0e4, 1.0e4
    targets[0, 0], targets[1, 1] = 40 * 56 + 7, 55 * 56 + 55                 # the -1e4 position (loss 2e4) and the +1e4 one (loss 0)
    out2, grad = check(cuda, heat, targets)
    assert bool(torch.isfinite(out2).all()) and bool(torch.isfinite(grad).all())


def test_maps_above_the_cap_are_refused_not_launched(cuda):
    from scda_amd import autograd_ops as A, native as N
    heat = torch.zeros(1, 1, 17, 241, device=cuda)                           # HW = 4097
    targets = torch.zeros(1, 1, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match="4096"):
        A.keypoint_heatmap_loss(heat, targets)
    buf = torch.zeros(8, device=cuda)
    status = N.lib().scda_keypoint_ce_fwd_hip(heat.data_ptr(), 4097, 4097, 1, 1, 4097, targets.data_ptr(), buf.data_ptr(), buf[2:].data_ptr(),
                                              buf[4:].data_ptr(), None)
    assert status != 0 and b"scda_keypoint_ce_fwd_hip" in N.lib().scda_last_error()
    with pytest.raises(ValueError, match="contiguous"):                      # a plane that is not contiguous is refused as well
        A.keypoint_heatmap_loss(torch.zeros(2, 2, 8, 16, device=cuda)[:, :, :, ::2], torch.zeros(2, 2, dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()


def test_autograd_function_returns_the_input_layout(cuda):
    from scda_amd import autograd_ops as A
    heat, targets = seeded((4, 3, 8, 8), 5)
    targets[2] = -1
    want, _, want_grad = ref64(heat, targets)
    x = heat.transpose(0, 1).contiguous().to(cuda).requires_grad_()          # the leaf is [Kp, R, h, w]; the loss sees its transpose
    loss = A.keypoint_heatmap_loss(x.transpose(0, 1), targets.to(cuda))
    (loss * 2.0).backward()
    assert abs(float(loss) - want) <= 1e-5 * abs(want)
    assert rel_l2(x.grad.transpose(0, 1), 2.0 * want_grad) <= 1e-4


_DET = {}


def keypoint_detector(cuda):
    """one seeded ResNet-50 detector with the training keypoint branch for the tests of this module"""
    if 'det' not in _DET:
        from scda_amd import resnet_config as RC
        from scda_amd.dropin.models.mask_rcnn.resnet import resnet50
        torch.manual_seed(3)
        shared = dict(RCFG['shared'], with_keypoint=True, num_keypoints=17, train_keypoint_target=dict(RC.KEYPOINT_TARGET))
        det = resnet50(cfg=shared)
        with torch.no_grad():
            for p in det.keypoint_head.parameters():
                if p.dim() == 1:
                    p.normal_(0, 0.05)                                       # biases: zero by construction, seeded here
        _DET['det'] = det.to(cuda).train()
    _DET['det'].zero_grad()
    return _DET['det']


def test_head_and_loss_match_torch_layers(cuda):
    """The HIP head (reference layout) + loss against F.conv2d / F.conv_transpose2d / F.interpolate / F.cross_entropy in float64: the
    loss within 1e-5, the 20 parameter gradients and the input gradient within 1e-4 relative L2.

    Two places where that comparison is not defined, and what is asserted there instead:
      * ReLU has no derivative at 0.  A pre-activation within float32 rounding of 0 has either sign on the device, and this loss's
        gradient is concentrated at the 50 targets, so ONE such element near a target decides 1e-3 of a gradient's norm (measured:
        2 of 4.8 M activations differ in sign from float64; the gradients below them are then off by 4e-5 and 1.2e-3, and by 7e-7 above
        them).  The float64 side therefore takes the device's sign where |z| <= 2^-17 rms(z) of its layer -- 128 float32 roundings of
        the layer's scale, 8 x the measured forward difference; about 6e-6 of the elements -- and its own everywhere else; the device's
        signs must equal float64's outside that band, and the band must stay that small.
      * The last bias: soft-max minus one-hot sums to zero over a map, so its exact gradient is 0.  Its error is measured against the
        norm of the per-channel sums of |d loss / d heat|, the terms it is the sum of."""
    import torch.nn.functional as F
    from scda_amd import autograd_ops as A
    det = keypoint_detector(cuda)
    head = det.keypoint_head
    names = [k for k, _ in head.named_parameters()]
    assert len(names) == 20
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 1024, 14, 14, generator=g)
    targets = torch.randint(0, 56 * 56, (4, 17), generator=g, dtype=torch.int32)
    targets[1, 3], targets[2] = -1, -1
    count = int((targets >= 0).sum())

    for m in head.modules():
        if hasattr(m, 'row_period'):
            m.row_period = 0
    signs = []
    hooks = [head[i].register_forward_hook(lambda mod, inp, out: signs.append((out > 0).cpu())) for i in range(9)]
    xd = x.to(cuda).requires_grad_()
    heat = head(xd)
    for h in hooks:
        h.remove()
    assert tuple(heat.shape) == (4, 17, 56, 56) and len(signs) == 9
    loss = A.keypoint_heatmap_loss(heat, targets.to(cuda))
    loss.backward()
    torch.cuda.synchronize()

    ref = {k: p.detach().cpu().double().requires_grad_() for k, p in head.named_parameters()}
    xr = x.double().requires_grad_()
    in_band = elements = 0

    def relu(z, device_sign):
        nonlocal in_band, elements
        band = z.detach().abs() <= 2.0 ** -17 * z.detach().pow(2).mean().sqrt()
        own = z.detach() > 0
        assert not ((own != device_sign) & ~band).any(), "a ReLU sign differs from float64 outside the rounding band"
        in_band, elements = in_band + int(band.sum()), elements + band.numel()
        return z * torch.where(band, device_sign, own).double()

    torch.set_num_threads(16)
    try:
        y = xr
        for i in range(8):
            y = relu(F.conv2d(y, ref["%d.0.weight" % i], ref["%d.0.bias" % i], padding=1), signs[i])
        y = relu(F.conv_transpose2d(y, ref["8.0.weight"], ref["8.0.bias"], stride=2), signs[8])
        y = F.interpolate(y, scale_factor=2, mode='bilinear', align_corners=True)
        y = F.conv2d(y, ref["10.weight"], ref["10.bias"])
        y.retain_grad()
        flat, t = y.reshape(4 * 17, 56 * 56), targets.reshape(-1).long()
        want = F.cross_entropy(flat[t >= 0], t[t >= 0], reduction='sum') / count
        want.backward()
    finally:
        torch.set_num_threads(1)
    assert in_band <= 1e-4 * elements, (in_band, elements)
    errs = {k: rel_l2(p.grad, ref[k].grad) for k, p in head.named_parameters() if k != "10.bias"}
    errs['input'] = rel_l2(xd.grad, xr.grad)
    terms = y.grad.abs().sum(dim=(0, 2, 3))
    errs['10.bias'] = float((head[10].bias.grad.detach().double().cpu() - ref["10.bias"].grad).norm() / terms.norm())
    print("keypoint head + loss vs torch fp64: loss %.8g vs %.8g, %d of %d activations in the rounding band, worst gradient %s"
          % (float(loss.detach()), float(want.detach()), in_band, elements, max(errs.items(), key=lambda kv: kv[1])))
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    assert len(errs) == 21 and max(errs.values()) <= 1e-4, errs


def _rois(n, seed=4):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand(n, generator=g) * 300; y1 = torch.rand(n, generator=g) * 200
    return torch.stack([torch.zeros(n), x1, y1, x1 + 20 + torch.rand(n, generator=g) * 150, y1 + 20 + torch.rand(n, generator=g) * 100], 1)


def test_channel_major_keypoint_branch_equals_reference_layout(cuda, monkeypatch):
    """the keypoint branch in training mode on the stacked view [1, C, R*14, 14] against the [R, C, 14, 14] batch: heat maps, the
    gradient into the backbone features, every parameter gradient (both sides on the direct kernels, as for the mask branch); then
    10 RoIs through the loss path, which pads them to 12 to stay on the stacked view, against the unpadded reference layout"""
    monkeypatch.setenv("SCDA_WINOGRAD", "0")
    from scda_amd import autograd_ops as A
    det = keypoint_detector(cuda)
    assert det.training
    feat = torch.randn(1, 1024, 20, 30, generator=torch.Generator().manual_seed(7)).to(cuda)
    rois = _rois(12)
    up = torch.randn(12, 17, 56, 56, generator=torch.Generator().manual_seed(8)).to(cuda)
    res = {}
    for tall in (False, True):
        det.tall_head = tall
        det.zero_grad()
        f = feat.clone().requires_grad_()
        y = det.keypoint_predictor(f, rois.to(cuda))
        assert tuple(y.shape) == (12, 17, 56, 56) and y.is_contiguous() != tall
        (y * up).sum().backward()
        res[tall] = (y.detach().clone(), f.grad.clone(), {k: p.grad.clone() for k, p in det.keypoint_head.named_parameters()})
    assert det.keypoint_roipooling.channel_major is True
    assert rel_l2(res[True][0], res[False][0]) <= 1e-5
    assert rel_l2(res[True][1], res[False][1]) <= 1e-5
    for k in res[True][2]:
        assert rel_l2(res[True][2][k], res[False][2][k]) <= 1e-5, k

    targets = torch.randint(0, 56 * 56, (10, 17), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    targets[4], targets[7, 2] = -1, -1
    # Both runs on ONE launch plan (128 x 128 tiles, no split-K, wherever that is legal).  Left to itself the planner splits K by the
    # pixel count, 10 and 12 RoIs get different K orders, activations differ in the last bit (7e-7) and a handful of 12 M pre-activations
    # next to 0 change sign; this loss's gradient is concentrated at the targets, so one such ReLU decides 5e-3 of the feature gradient
    # (measured).  With equal plans the forward passes are the same sums and the comparison is about the padding alone.
    monkeypatch.setenv("SCDA_PLAN_FORCE", "128,128,1")
    res = {}
    for tall in (False, True):
        det.tall_head = tall
        det.zero_grad()
        f = feat.clone().requires_grad_()
        loss = det._keypoint_loss(f, rois[:10], targets)
        loss.backward()
        assert det.last_keypoint_rois == (12 if tall else 10) and det.keypoint_roipooling.channel_major is tall
        res[tall] = (float(loss), f.grad.clone(), {k: p.grad.clone() for k, p in det.keypoint_head.named_parameters()})
    # the unpadded reference-layout run is the composition the loss path states: predictor, then the loss
    det.tall_head = False
    heat = det.keypoint_predictor(feat, rois[:10].to(cuda)).detach()
    assert abs(float(A.keypoint_heatmap_loss(heat, targets.to(cuda))) - res[False][0]) <= 1e-6 * abs(res[False][0])
    det.tall_head = True
    assert abs(res[True][0] - res[False][0]) <= 1e-5 * abs(res[False][0])
    assert rel_l2(res[True][1], res[False][1]) <= 1e-5
    for k in res[True][2]:
        if k != "10.bias":
            assert rel_l2(res[True][2][k], res[False][2][k]) <= 1e-5, k
    # the last bias: soft-max minus one-hot sums to zero over a map, its exact gradient is 0 and both sides hold rounding only; the
    # scale is that of the terms it sums, per channel sum over counted RoIs of 2 (1 - p[target]) / count
    on = (targets >= 0).to(cuda)
    p_t = torch.softmax(heat.reshape(10, 17, -1).double(), dim=2).gather(2, targets.clamp(min=0).long().to(cuda)[..., None])[..., 0]
    terms = (2.0 * (1.0 - p_t) * on).sum(dim=0) / on.sum()
    assert float((res[True][2]["10.bias"] - res[False][2]["10.bias"]).double().norm() / terms.norm()) <= 1e-5


def _finite(out):
    return all(bool(torch.isfinite(v).all()) for v in out.values() if torch.is_tensor(v))


def test_keypoint_scda_iteration_at_800x1344(cuda):
    """the configuration's own size: two full SCDA iterations with the keypoint loss -- finite losses, the keypoint head and the
    backbone behind it move, the RoI list is a multiple of 4 within the quota"""
    import bench
    from scda_amd import resnet_config as RC
    torch.manual_seed(0); np.random.seed(0)
    tr = RC.make_trainer(bench.CFG, cuda, lr=1e-4, with_keypoint=True)
    det = tr.model
    before = {k: v.clone() for k, v in det.state_dict().items()}
    src, tgt, gts, info = bench.synth_batch(0, RC.H, RC.W)
    kps = RC.synth_keypoints(gts, 17, seed=0)
    for _ in range(2):
        out = tr.step(src.to(cuda), gts, info, tgt.to(cuda), gt_keypoints=kps)
    torch.cuda.synchronize()
    assert _finite(out), out
    assert float(out['keypoint_loss']) > 0.0 and 'mask_loss' not in out
    G = gts.shape[1]
    assert G <= det.last_keypoint_rois <= RC.KEYPOINT_ROIS and det.last_keypoint_rois % 4 == 0
    after = det.state_dict()
    moved = [k for k in before if k.startswith('keypoint_head') and not torch.equal(before[k], after[k])]
    assert len(moved) == 20, moved
    assert not torch.equal(before['layer3.5.conv3.weight'], after['layer3.5.conv3.weight'])
    assert torch.equal(before['layer1.0.conv1.weight'], after['layer1.0.conv1.weight'])


def test_both_branches_report_six_losses(cuda):
    import bench
    from scda_amd import resnet_config as RC
    torch.manual_seed(0); np.random.seed(0)
    tr = RC.make_trainer(bench.CFG, cuda, lr=1e-4, with_mask=True, mask_iou=0.2, with_keypoint=True)
    seen = []
    tr.model.register_forward_hook(lambda m, i, o: seen.append(len(o['losses'])))
    src, tgt, gts, info = bench.synth_batch(0, RC.H, RC.W)
    out = tr.step(src.to(cuda), gts, info, tgt.to(cuda), gt_masks=RC.synth_masks(gts), gt_keypoints=RC.synth_keypoints(gts, 17, seed=0))
    torch.cuda.synchronize()
    assert seen == [6] and tr.model.last_extra_loss_names == ('mask_loss', 'keypoint_loss')
    assert _finite(out) and float(out['mask_loss']) > 0.0 and float(out['keypoint_loss']) > 0.0


def test_stepping_without_keypoints_trains_the_other_losses(cuda):
    import bench
    from scda_amd import resnet_config as RC
    torch.manual_seed(0); np.random.seed(0)
    tr = RC.make_trainer(bench.CFG, cuda, lr=1e-4, with_keypoint=True)
    before = tr.model.state_dict()['layer3.5.conv3.weight'].clone()
    src, tgt, gts, info = bench.synth_batch(0, RC.H, RC.W)
    out = tr.step(src.to(cuda), gts, info, tgt.to(cuda))
    torch.cuda.synchronize()
    assert _finite(out) and 'keypoint_loss' not in out and 'mask_loss' not in out and float(out['rcnn_cls']) > 0.0
    assert tr.model.last_extra_loss_names == ()
    assert not torch.equal(before, tr.model.state_dict()['layer3.5.conv3.weight'])
