"""ringdp.nn.DepthwiseConv2d on CPU tensors: the ATen oracle path on channels-last activations."""
import torch
import torch.nn.functional as F

import ringdp.nn


def test_cpu_module_equals_permuted_conv2d():
    torch.manual_seed(0)
    N, H, W, C, K = 2, 9, 11, 16, 7
    mod = ringdp.nn.DepthwiseConv2d(C, K)
    assert mod.weight.shape == (C, 1, K, K) and mod.bias.shape == (C,)
    x = torch.randn(N, H, W, C, requires_grad=True)
    dy = torch.randn(N, H, W, C)
    y = mod(x)
    assert y.shape == (N, H, W, C)
    got = torch.autograd.grad(y, (x, mod.weight, mod.bias), dy)
    xr = x.detach().clone().requires_grad_()
    wr, br = mod.weight.detach().clone().requires_grad_(), mod.bias.detach().clone().requires_grad_()
    yr = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=K // 2, groups=C).permute(0, 2, 3, 1)
    ref = torch.autograd.grad(yr, (xr, wr, br), dy)
    assert torch.equal(y, yr)
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_exported_and_state_dict_compatible():
    assert "DepthwiseConv2d" in ringdp.nn.__all__ and "depthwise_conv2d" in ringdp.nn.__all__
    conv = torch.nn.Conv2d(24, 24, 7, padding=3, groups=24, bias=False)
    mod = ringdp.nn.DepthwiseConv2d(24, 7, bias=False)
    mod.load_state_dict(conv.state_dict())
    assert mod.bias is None and torch.equal(mod.weight, conv.weight)
