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
