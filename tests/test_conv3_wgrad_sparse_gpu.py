"""The sparse-MFMA conv3 weight gradient of the 8-wave backward (conv3_wgrad8_role) on constructed inputs.

The backward takes the pool3 argmax bytes and a3 as inputs, so every argmax pattern can be forced: all windows
at position 0, 1, 2 or 3 (the sparse instruction's index values), random positions, and dead windows (a3 <= 0:
no live value in the group of four).  Oracles: the dense 4-wave kernel on chunks of at most 2048 images (dz2
bit-identical, weight gradients within 1e-5 relative norm: another fp32 order), and for dw3 a float64 ATen
product of the same bf16 operands (bound 5e-3 of the largest entry, as test_conv3_fc_backward)."""
import functools
import os

import pytest
import torch

from test_convnet_kernels_gpu import C, bf, packed, pool2_ref, unpool2x2, weights

pytestmark = pytest.mark.gpu

CHUNK = 2048  # largest batch of the 4-wave kernel
B_MIN8 = CHUNK + 1  # smallest 8-wave batch: 18-19 images per wgrad slice (every residue of the 3-buffer ring)
DGRAD_FRAC, STEAL = 0.66, 0.04  # the defaults of c3_split() / c3_dgrad_images()


def steal_batch():
    """Smallest round batch at which the wgrad workgroups go on to the data gradient of the batch's tail:
    B >= 32 * n_dgrad, n_dgrad as c3_split() derives it from the CU count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frac = float(os.environ.get("RINGDP_C3_DGRAD_FRAC", DGRAD_FRAC))
    nd = min(max((int(frac * cus) + 4) // 8 * 8, 8), cus - 8)
    B = -(-32 * nd // 100) * 100
    steal = float(os.environ.get("RINGDP_C3_STEAL", STEAL))
    assert B > CHUNK and B >= 32 * nd and int(steal * B) > 0, (cus, nd, B)
    return B


def batch(which):
    return B_MIN8 if which == "min8" else steal_batch()


@functools.lru_cache(maxsize=None)
def base(B):
    torch.manual_seed(300 + B)
    dev = torch.device("cuda")
    ws = weights(dev, 23)
    z2 = torch.randn(B, 11, 11, 64, device=dev).bfloat16()
    a2, idx2 = pool2_ref(z2)
    dl = torch.randn(B, 10, device=dev)
    return ws, packed(ws), a2, idx2, dl


@functools.lru_cache(maxsize=None)
def case(B, argmax, dead):
    ws, pk, a2, idx2, dl = base(B)
    g = torch.Generator(device="cuda").manual_seed(B + 7 * len(argmax) + dead)
    if argmax == "random":
        idx3 = torch.randint(0, 4, (B, 16, 128), device="cuda", generator=g, dtype=torch.uint8)
    else:
        idx3 = torch.full((B, 16, 128), int(argmax), device="cuda", dtype=torch.uint8)
    a3 = torch.randn(B, 16, 128, device="cuda", generator=g)  # about half <= 0: dead windows
    if not dead:
        a3 = a3.abs() + 0.01
    a3 = a3.bfloat16()
    assert bool((a3 > 0).all()) != bool(dead)
    return ws, pk, a2, idx2, a3, idx3, dl


def backward(key, lo, hi, need_dz2=True):
    ws, pk, a2, idx2, a3, idx3, dl = case(*key)
    g = [torch.empty_like(ws[i]) for i in (4, 5, 6, 7)]
    dz2 = C().cn_conv3_fc_bwd(a2[lo:hi].contiguous(), idx2[lo:hi].contiguous(), a3[lo:hi].contiguous(),
                              idx3[lo:hi].contiguous(), ws[6], dl[lo:hi].contiguous(), pk, need_dz2, *g)
    torch.cuda.synchronize()
    return dz2, g


@functools.lru_cache(maxsize=None)
def whole(key):
    return backward(key, 0, key[0])


def dw3_float64(key):
    """dW3[co][ci][ky][kx] = sum d(conv3)[b][y][x][co] * a2[b][y+ky][x+kx][ci] in float64 (ATen matmuls), from the
    operands the kernels multiply: a2 and the bf16 d(conv3) that the fc1 backward leaves (bf16 fc1 weights)."""
    ws, _, a2, _, a3, idx3, dl = case(*key)
    B = key[0]
    da3 = (dl @ bf(ws[6])).view(B, 128, 4, 4).permute(0, 2, 3, 1)
    dconv = bf(unpool2x2(da3, idx3.view(B, 4, 4, 128), a3.view(B, 4, 4, 128), 8)).double().reshape(B * 64, 128)
    a2d = a2.double()
    out = torch.empty(128, 64, 3, 3, dtype=torch.float64, device=a2.device)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = dconv.t() @ a2d[:, ky:ky + 8, kx:kx + 8, :].reshape(B * 64, 64)
    return out


@pytest.mark.parametrize("which", ["min8", "steal"])
@pytest.mark.parametrize("dead", [0, 1])
@pytest.mark.parametrize("argmax", ["0", "1", "2", "3", "random"])
def test_against_dense_chunks_and_float64(argmax, dead, which):
    B = batch(which)
    key = (B, argmax, dead)
    dz2, g = whole(key)
    assert dz2.shape == (B, 11, 11, 64)
    sums = [torch.zeros_like(t, dtype=torch.float64) for t in g]
    for lo in range(0, B, CHUNK):
        hi = min(lo + CHUNK, B)
        dz2_c, g_c = backward(key, lo, hi)
        assert torch.equal(dz2_c, dz2[lo:hi]), (lo, hi)
        for s, t in zip(sums, g_c):
            s += t.double()
    for name, s, t in zip(("dw3", "db3", "dWfc", "dbfc"), sums, g):
        err = float((s - t.double()).norm() / t.double().norm())
        print(name, "vs dense chunks, relative norm", err)
        assert err < 1e-5, name
    ref = dw3_float64(key)
    err = float((g[0].double() - ref).abs().max() / ref.abs().max())
    print("dw3 vs float64, max error / max entry", err)
    assert err < 5e-3


def test_deterministic():
    key = (steal_batch(), "random", 1)
    dz2, g = whole(key)
    dz2_b, g_b = backward(key, 0, key[0])
    assert torch.equal(dz2, dz2_b)
    for a, b in zip(g, g_b):
        assert torch.equal(a, b)


def test_weight_gradients_without_dz2():
    key = (B_MIN8, "random", 1)
    _, g = whole(key)
    dz2, g_w = backward(key, 0, B_MIN8, need_dz2=False)
    assert dz2 is None
    for a, b in zip(g_w, g):
        assert torch.equal(a, b)
