"""The fc1 head at the smallest separate-launch batches: no result may depend on which workgroup of
fc1_fwd_kernel or fc_bwd_kernel takes which image group, nor on the cache policy of the dz2 stores of the 8-wave
conv3 backward (nontemporal; the 4-wave path's are plain).  Written with the round that measured both passes
over a3 in either direction (profiles/r15/head_bytes/README.md; the order stayed as it was).

B = 2049, 2300 and 4129 give fc_bwd_kernel 32 images per workgroup and a last image group of 1, 28 and 1
images; 4129 is also above the batch up to which fc1 runs inside conv3's forward launch, so its logits come
from fc1_fwd_kernel (33 workgroups, the last with 3 groups of 16 images, the last group with 1 image).
Oracles: the 4-wave path on chunks of at most 2048 images, where the fc1 backward runs inside the conv3 launch
(dz2 bit-identical; fc1 weight, fc1 bias and conv3 bias gradients within 1e-5 relative norm of the chunks' sum,
the bound of test_conv3_wgrad_sparse_gpu: another fp32 order), and for the logits a float64 product of the same
bf16 operands at test_conv3_fc_forward's tolerance."""
import functools

import pytest
import torch

from test_convnet_kernels_gpu import C, bf, packed, pool2_ref, rel_err, weights

pytestmark = pytest.mark.gpu

CHUNK = 2048  # largest batch of the 4-wave kernel
BATCHES = [2049, 2300, 4129]


@functools.lru_cache(maxsize=None)
def case(B):
    torch.manual_seed(500 + B)
    dev = torch.device("cuda")
    ws = weights(dev, 31)
    z2 = torch.randn(B, 11, 11, 64, device=dev).bfloat16()
    a2, idx2 = pool2_ref(z2)
    dl = torch.randn(B, 10, device=dev)
    return ws, packed(ws), a2, idx2, dl


def forward(B):
    ws, pk, a2, _, _ = case(B)
    out = C().cn_conv3_fc_fwd(a2, pk, ws[5], ws[7])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def activations(B):
    return forward(B)


def backward(B, lo, hi):
    ws, pk, a2, idx2, dl = case(B)
    _, a3, idx3 = activations(B)
    g = [torch.empty_like(ws[i]) for i in (4, 5, 6, 7)]
    dz2 = C().cn_conv3_fc_bwd(a2[lo:hi].contiguous(), idx2[lo:hi].contiguous(), a3[lo:hi].contiguous(),
                              idx3[lo:hi].contiguous(), ws[6], dl[lo:hi].contiguous(), pk, True, *g)
    torch.cuda.synchronize()
    return dz2, g


@functools.lru_cache(maxsize=None)
def whole(B):
    return backward(B, 0, B)


@pytest.mark.parametrize("B", BATCHES)
def test_whole_batch_against_chunks(B):
    dz2, g = whole(B)
    assert dz2.shape == (B, 11, 11, 64)
    sums = [torch.zeros_like(t, dtype=torch.float64) for t in g]
    for lo in range(0, B, CHUNK):
        hi = min(lo + CHUNK, B)
        dz2_c, g_c = backward(B, lo, hi)
        assert torch.equal(dz2_c, dz2[lo:hi]), (lo, hi)
        for s, t in zip(sums, g_c):
            s += t.double()
    for name, s, t in list(zip(("dw3", "db3", "dWfc", "dbfc"), sums, g))[1:]:
        err = float((s - t.double()).norm() / t.double().norm())
        print(name, "vs chunks, relative norm", err)
        assert err <= 1e-5, name


@pytest.mark.parametrize("B", BATCHES)
def test_two_runs_byte_equal(B):
    dz2, g = whole(B)
    dz2_b, g_b = backward(B, 0, B)
    assert torch.equal(dz2, dz2_b)
    for a, b in zip(g, g_b):
        assert torch.equal(a, b)
    for a, b in zip(activations(B), forward(B)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B", BATCHES)
def test_logits_against_float64(B):
    ws = case(B)[0]
    logits, a3, _ = activations(B)
    a3_flat = a3.view(B, 4, 4, 128).permute(0, 3, 1, 2).reshape(B, 2048).double()
    ref = a3_flat @ bf(ws[6]).double().t() + ws[7].double()
    err = rel_err(logits, ref)
    print("logits vs float64, max error / max entry", err)
    assert err < 1.5e-2
