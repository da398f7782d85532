"""The 8-wave conv3 backward (conv3_bwd8_kernel, batches above 2048) against the 4-wave kernel.

Both kernels form dz2 with the same expressions in the same order and dz2 of an image depends on that image
alone, so a batch run whole (8-wave) and in chunks of at most 2048 images (4-wave) gives the same dz2 bits,
and weight gradients that differ by the slab partition only (other fp32 summation order)."""
import functools
import os

import pytest
import torch

from test_convnet_kernels_gpu import C, packed, pool2_ref, weights

pytestmark = pytest.mark.gpu

CHUNK = 2048  # largest batch of the 4-wave kernel (fc_in_c3_max_batch)
B_MIN8 = CHUNK + 1  # smallest batch of the 8-wave kernel: 14-15 images per dgrad workgroup, 18-19 per wgrad slice


def steal_batch():
    """Smallest round batch at which the wgrad workgroups take the data gradient of the batch's tail (the
    'steal'): B >= 32 * n_dgrad, n_dgrad as c3_split() derives it from the CU count."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frac = float(os.environ.get("RINGDP_C3_DGRAD_FRAC", 0.55))
    nd = min(max((int(frac * cus) + 4) // 8 * 8, 8), cus - 8)
    B = -(-32 * nd // 100) * 100
    steal = float(os.environ.get("RINGDP_C3_STEAL", 0.04))
    assert B > CHUNK and B >= 32 * nd and int(steal * B) > 0, (cus, nd, B)
    return B


@functools.lru_cache(maxsize=None)
def case(B):
    torch.manual_seed(100 + B)
    dev = torch.device("cuda")
    ws = weights(dev, 17)
    pk = packed(ws)
    z2 = torch.randn(B, 11, 11, 64, device=dev).bfloat16()
    a2, idx2 = pool2_ref(z2)
    _, a3, idx3 = C().cn_conv3_fc_fwd(a2, pk, ws[5], ws[7])
    dl = torch.randn(B, 10, device=dev)
    return ws, pk, a2, idx2, a3, idx3, dl


def backward(B, lo, hi, need_dz2=True):
    ws, pk, a2, idx2, a3, idx3, dl = case(B)
    g = [torch.empty_like(ws[i]) for i in (4, 5, 6, 7)]
    dz2 = C().cn_conv3_fc_bwd(a2[lo:hi].contiguous(), idx2[lo:hi].contiguous(), a3[lo:hi].contiguous(),
                              idx3[lo:hi].contiguous(), ws[6], dl[lo:hi].contiguous(), pk, need_dz2, *g)
    torch.cuda.synchronize()
    return dz2, g


@functools.lru_cache(maxsize=None)
def whole(B):
    return backward(B, 0, B)


@pytest.mark.parametrize("which", ["min8", "steal"])
def test_chunks_bit_identical(which):
    B = B_MIN8 if which == "min8" else steal_batch()
    dz2, g = whole(B)
    assert dz2.shape == (B, 11, 11, 64)
    sums = [torch.zeros_like(t, dtype=torch.float64) for t in g]
    for lo in range(0, B, CHUNK):
        hi = min(lo + CHUNK, B)
        dz2_c, g_c = backward(B, lo, hi)
        assert torch.equal(dz2_c, dz2[lo:hi]), (lo, hi)
        for s, t in zip(sums, g_c):
            s += t.double()
    for name, s, t in zip(("dw3", "db3", "dWfc", "dbfc"), sums, g):
        err = float((s - t.double()).norm() / t.double().norm())
        print(name, err)
        assert err < 1e-5, name


def test_weight_gradients_without_dz2():
    """need_dz2=False returns no dz2 and byte-equal weight gradients: c3_split() gives both calls the same
    wgrad slices, hence the same slabs and the same fp32 summation order."""
    _, g = whole(B_MIN8)
    dz2, g_w = backward(B_MIN8, 0, B_MIN8, need_dz2=False)
    assert dz2 is None
    for name, a, b in zip(("dw3", "db3", "dWfc", "dbfc"), g_w, g):
        print(name, torch.equal(a, b), float((a - b).norm() / b.norm()))
    for a, b in zip(g_w, g):
        assert torch.equal(a, b)


def test_deterministic():
    B = steal_batch()
    dz2, g = whole(B)
    dz2_b, g_b = backward(B, 0, B)
    assert torch.equal(dz2, dz2_b)
    for a, b in zip(g, g_b):
        assert torch.equal(a, b)
