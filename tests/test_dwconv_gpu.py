"""Depthwise K x K convolution on NHWC bf16 (csrc/kernels/dwconv.hip): forward, data gradient, weight and bias
gradient against fp64 ``F.conv2d(groups=C)`` and its autograd on the same bf16 inputs and fp32 parameters.

Bounds (derived, not tuned).  bf16 outputs: ``|got - ref| <= 2^-8 |ref| + 2^-16 A`` with ``A`` the same sum over
absolute values (half a bf16 ulp for the single rounding, plus fp32 accumulation of at most 50 terms with ~20x margin).
fp32 outputs: ``|got - ref| <= L 2^-24 A_w`` with ``L = N H W`` terms, the worst case of any fp32 summation order."""
import pytest
import torch
import torch.nn.functional as F

import ringdp.nn
from ringdp._native import C as _C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = [  # N, H, W, C, K
    (2, 9, 11, 40, 7),    # C no multiple of any slab, H and W below every tile, odd sizes
    (1, 20, 37, 32, 7),   # crosses a column-tile and a row-tile edge, halo rows shared between tiles
    (3, 7, 7, 128, 7),    # the small-map mapping: the whole image is one tile
    (2, 2, 3, 8, 7),      # the image is smaller than the kernel
    (2, 14, 14, 64, 3),
    (2, 14, 14, 64, 5),
    (5, 16, 16, 16, 7),   # a weight-gradient workgroup walks over several images
]


def _inputs(N, H, W, Cc, K):
    g = torch.Generator().manual_seed(1000 * N + 100 * K + H * W + Cc)
    x = torch.randn(N, H, W, Cc, generator=g).bfloat16()
    dy = torch.randn(N, H, W, Cc, generator=g).bfloat16()
    return x, torch.randn(Cc, 1, K, K, generator=g) * 0.2, torch.randn(Cc, generator=g), dy


def reference(x, w, b, dy):
    """fp64 (y, dx, dw, db), then the same four sums over absolute values (the A of the bounds); y and dx in NHWC."""
    def run(x, w, b, dy):
        x, w, b = (t.double().requires_grad_() for t in (x.permute(0, 3, 1, 2), w, b))
        y = F.conv2d(x, w, b, padding=w.shape[-1] // 2, groups=w.shape[0])
        dx, dw, db = torch.autograd.grad(y, (x, w, b), dy.double().permute(0, 3, 1, 2))
        return y.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw, db

    return run(x, w, b, dy), run(x.abs(), w.abs(), b.abs(), dy.abs())


def check(name, got, ref, A, L=None):
    """L = None: a bf16 output; else an fp32 sum of L terms."""
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * A if L is None else L * 2.0 ** -24 * A
    err = (got.cpu().double() - ref).abs()
    print(f"{name}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert got.shape == ref.shape and bool((err <= bound).all()), name


@pytest.mark.parametrize("N,H,W,Cc,K", CASES)
def test_kernels_against_fp64(N, H, W, Cc, K):
    x, w, b, dy = _inputs(N, H, W, Cc, K)
    (y, dx, dw, db), (Ay, Adx, Aw, Ab) = reference(x, w, b, dy)
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    check("y", _C.dwconv_fwd(xd, wd, bd, False), y, Ay)
    check("dx", _C.dwconv_fwd(dyd, wd, None, True), dx, Adx)
    got_dw, got_db = _C.dwconv_wgrad(xd, dyd, K, True)
    check("dw", got_dw, dw, Aw, N * H * W)
    check("db", got_db, db, Ab, N * H * W)
    assert _C.dwconv_wgrad(xd, dyd, K, False)[1] is None


def test_wgrad_is_deterministic():
    x, _, _, dy = _inputs(3, 20, 37, 40, 7)
    xd, dyd = x.to(DEV), dy.to(DEV)
    dw0, db0 = _C.dwconv_wgrad(xd, dyd, 7, True)
    dw1, db1 = _C.dwconv_wgrad(xd, dyd, 7, True)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)


def test_module_loads_conv2d_state_and_trains():
    N, H, W, Cc, K = CASES[0]
    x, _, _, dy = _inputs(N, H, W, Cc, K)
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(Cc, Cc, K, padding=K // 2, groups=Cc)
    mod = ringdp.nn.DepthwiseConv2d(Cc, K)
    mod.load_state_dict(conv.state_dict())
    mod.to(DEV)
    (y, dx, dw, db), (Ay, Adx, Aw, Ab) = reference(x, conv.weight.detach(), conv.bias.detach(), dy)
    xd = x.to(DEV).requires_grad_()
    out = mod(xd)
    (out.float() * dy.to(DEV).float()).sum().backward()
    assert out.dtype == torch.bfloat16 and mod.weight.dtype == torch.float32
    check("y", out.detach(), y, Ay)
    check("dx", xd.grad, dx, Adx)
    check("dw", mod.weight.grad, dw, Aw, N * H * W)
    check("db", mod.bias.grad, db, Ab, N * H * W)


@pytest.mark.parametrize("what", ["C=12", "K=4", "non-contiguous"])
def test_rejects(what):
    Cc, K = (12 if what == "C=12" else 16), (4 if what == "K=4" else 7)
    x = torch.zeros(2, 8, 8, Cc, device=DEV, dtype=torch.bfloat16)
    if what == "non-contiguous":
        x = x.transpose(1, 2)
    w, b = torch.zeros(Cc, 1, K, K, device=DEV), torch.zeros(Cc, device=DEV)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        _C.dwconv_fwd(x, w, b, False)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        _C.dwconv_wgrad(x, x, K, True)
