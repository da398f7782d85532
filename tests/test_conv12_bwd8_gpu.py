"""The 8-wave conv2 backward + conv1 weight gradient (conv12_bwd8_kernel, batches above 2048) against the
4-wave kernel.

A batch run whole (8-wave) and in chunks of at most 2048 images (4-wave) forms the same per-image products;
the weight gradients differ by the slab partition and the k-step partition only (other fp32 summation order).
2049 is the smallest batch the 8-wave kernel sees: 13-14 images per dgrad workgroup and 19-20 per wgrad slice
on 256 CUs at the default split (152 + 104 workgroups), 2300 gives 15-16 and 22-23, so both parities of the
by-two unrolled steps and all three ring slots occur in every workgroup.

Measured relative norms (bound 1e-4): dw2 3.4e-7 .. 4.3e-7, db2 1.1e-7 .. 1.4e-7, dw1 1.9e-7 .. 2.3e-7,
db1 0.9e-7 .. 1.5e-7, before and after conv1's k-steps were shared with the MFMA waves."""
import functools

import pytest
import torch

from test_convnet_kernels_gpu import C, input_batch, packed, weights

pytestmark = pytest.mark.gpu

CHUNK = 2048  # largest batch of the 4-wave kernel (fc_in_c3_max_batch)
BOUND = 1e-4  # relative norm: test_conv12_backward_fused's bound for the fused 8-wave / separate-kernel pair
NAMES = ("dw2", "db2", "dw1", "db1")


@functools.lru_cache(maxsize=None)
def case(B, u8):
    torch.manual_seed(200 + B + u8)
    dev = torch.device("cuda")
    ws = weights(dev, 23)
    pk = packed(ws)
    x, _, norm = input_batch(B, u8, dev)
    a1, idx1 = C().cn_conv1_fwd(x, pk, ws[1], *norm)
    dz2 = torch.randn(B, 11, 11, 64, device=dev).bfloat16()
    return ws, pk, x, a1, idx1, dz2, norm


def backward(B, u8, lo, hi):
    ws, pk, x, a1, idx1, dz2, norm = case(B, u8)
    g = [torch.empty_like(ws[i]) for i in (2, 3, 0, 1)]
    C().cn_conv12_bwd(x[lo:hi].contiguous(), idx1[lo:hi].contiguous(), a1[lo:hi].contiguous(),
                      dz2[lo:hi].contiguous(), pk, *g, *norm)
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def whole(B, u8):
    return backward(B, u8, 0, B)


@pytest.mark.parametrize("B", [CHUNK + 1, 2300])
@pytest.mark.parametrize("u8", [True, False])
def test_whole_batch_against_chunks(B, u8):
    g = whole(B, u8)
    sums = [torch.zeros_like(t, dtype=torch.float64) for t in g]
    for lo in range(0, B, CHUNK):
        for s, t in zip(sums, backward(B, u8, lo, min(lo + CHUNK, B))):
            s += t.double()
    errs = [float((s - t.double()).norm() / t.double().norm()) for s, t in zip(sums, g)]
    for name, err in zip(NAMES, errs):
        print(f"B={B} u8={u8} {name} {err:.3e}")
    for name, err in zip(NAMES, errs):
        assert err < BOUND, name


def test_deterministic():
    g = whole(2300, True)
    g_b = backward(2300, True, 0, 2300)
    for name, a, b in zip(NAMES, g, g_b):
        assert torch.equal(a, b), name
