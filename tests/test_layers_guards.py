"""Argument guards of scda_amd.layers that sit in front of every kernel launch: no device needed."""
import pytest
import torch


def test_batch_norm_training_refuses_one_value_per_channel():
    """as torch: with B * H * W == 1 the unbiased running variance would be n / (n - 1) = 1 / 0"""
    from scda_amd import layers as L
    x = torch.randn(1, 3, 1, 1)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        L.BatchNorm2d(3).train()(x)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        torch.nn.BatchNorm2d(3).train()(x)


@pytest.mark.parametrize("kw", [dict(output_padding=1), dict(groups=2), dict(dilation=2), dict(groups=4, dilation=2)],
                         ids=lambda kw: ",".join(kw))
def test_transposed_convolutions_refuse_what_they_would_ignore(kw):
    """the two transposed convolutions read one dense [in, out, k, k] weight with one tap per output pixel: output_padding, groups and
    dilation are refused at construction, as layers.Conv2d refuses its own"""
    from scda_amd import layers as L
    with pytest.raises(NotImplementedError, match="ConvTranspose2x2s2"):
        L.ConvTranspose2x2s2(16, 4, **kw)
    with pytest.raises(NotImplementedError, match="ConvTranspose1x1"):
        L.ConvTranspose1x1(16, 4, **kw)
    with pytest.raises(NotImplementedError):
        L.Conv2d(16, 4, 3, **{k: v for k, v in kw.items() if k != "output_padding"} or dict(groups=2))
    assert L.ConvTranspose1x1(16, 4).weight.shape == (16, 4, 1, 1) and L.ConvTranspose2x2s2(16, 4, bias=False).bias is None


def test_batch_norm_refuses_another_channel_count():
    """the kernels size every per-channel read and the running-statistics update by the input's channels, not by the module's"""
    from scda_amd import layers as L
    for bn in (L.BatchNorm2d(4).train(), L.BatchNorm2d(4).eval()):
        before = (bn.running_mean.clone(), bn.running_var.clone())
        with pytest.raises(ValueError, match="expected a"):
            bn(torch.randn(2, 8, 3, 3))
        with pytest.raises(ValueError, match="expected a"):
            bn.forward_add_relu(torch.randn(1, 8, 4, 4), torch.randn(1, 8, 4, 4))
        with pytest.raises(ValueError, match="expected a"):
            bn(torch.randn(2, 4, 9))
        assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
