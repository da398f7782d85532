"""conv1's weight gradient on the sparse MFMA (the dgrad role of conv12_bwd8_kernel, batches above 2048) against
the dense 4-wave kernel and the ATen product.

The pool1 codes are built directly ([B, 13 py, 16 co/2, 16 px] bytes, low nibble the even channel, one-hot
1 << (dy * 2 + dx), px 13..15 zero), so that every argmax and ReLU-dead windows (nibble 0) occur where the test
wants them; a1 is positive exactly where the code is non-zero, as the ATen oracle masks by a1 > 0.  da1 is formed
inside the kernel from dz2 and is not masked: a dead window, or a live one in the other row half, must contribute
nothing through the value, whatever its index says.

Oracles: the dense 4-wave kernel on chunks of at most 2048 images summed in float64 (dw1, db1 below 1e-5 relative
norm: one misplaced term at B = 2049 moves it by about 1e-4; dw2, db2 below 1e-4 as in test_conv12_bwd8_gpu.py),
and for the random cases the float32 ATen product built as test_conv12_backward_fused does (1.5e-2 of the largest
entry).  Batches 2049 (uint8 input) and 2300 (float input): both parities of the by-two unrolled steps and all
three ring slots occur in every workgroup.

Measured relative norms at the committed split (144 + 112 workgroups): against the dense kernel dw1 1.8e-7 ..
2.6e-7, db1 0.8e-7 .. 1.5e-7, dw2 2.8e-7 .. 4.7e-7, db2 1.0e-7 .. 1.5e-7; against ATen dw1 2.2e-5 .. 4.3e-5,
db1 2.0e-5 .. 3.8e-5 of the largest entry; one image dw1 4.5e-8 .. 5.5e-8, db1 0 (26 cases, 18 s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_convnet_kernels_gpu import C, bf, conv1_codes, input_batch, packed, rel_err, unpool2x2, weights

pytestmark = pytest.mark.gpu

CHUNK = 2048     # largest batch of the 4-wave kernel
BOUND1 = 1e-5    # dw1, db1 against the dense kernel, relative norm
BOUND2 = 1e-4    # dw2, db2 against the dense kernel, relative norm
BOUND_ATEN = 1.5e-2
NAMES = ("dw2", "db2", "dw1", "db1")
BATCHES = [CHUNK + 1, 2300]
ARGMAX = [0, 1, 2, 3, "random"]


def make_codes(arg, live):
    """arg [B,13,13,32] in 0..3, live [B,13,13,32] bool (NHWC like a1) -> code rows [B,13,16,16] bytes."""
    nib = torch.where(live, torch.ones_like(arg) << arg, torch.zeros_like(arg)).permute(0, 1, 3, 2)  # [B,py,co,px]
    idx = torch.zeros(arg.shape[0], 13, 16, 16, dtype=torch.uint8, device=arg.device)
    idx[..., :13] = nib[:, :, 0::2] | (nib[:, :, 1::2] << 4)
    return idx


@functools.lru_cache(maxsize=None)
def case(B, argmax, dead):
    """dead: 0 no dead window, 1 half of them, 2 all."""
    u8 = B == CHUNK + 1
    torch.manual_seed(300 + B + 7 * ARGMAX.index(argmax) + dead)
    dev = torch.device("cuda")
    ws = weights(dev, 29)
    pk = packed(ws)
    x, xn, norm = input_batch(B, u8, dev)
    shape = (B, 13, 13, 32)
    if argmax == "random":
        arg = torch.randint(0, 4, shape, dtype=torch.uint8, device=dev)
    else:
        arg = torch.full(shape, argmax, dtype=torch.uint8, device=dev)
    # the a1 and the liveness of the "no dead window" twin: an all-dead call differs from it in the codes only
    a1_full = (torch.rand(shape, device=dev) + 0.1).bfloat16()
    live = {0: torch.ones(shape, dtype=torch.bool, device=dev), 1: torch.rand(shape, device=dev) < 0.5,
            2: torch.zeros(shape, dtype=torch.bool, device=dev)}[dead]
    idx1 = make_codes(arg, live)
    assert torch.equal(conv1_codes(idx1), torch.where(live, arg | 4, torch.zeros_like(arg)))
    a1 = a1_full if dead == 2 else torch.where(live, a1_full, torch.zeros_like(a1_full))
    dz2 = torch.randn(B, 11, 11, 64, device=dev).bfloat16()
    return ws, pk, x, xn, a1, idx1, dz2, norm, arg, live


def backward(c, lo, hi, dz2=None, idx1=None):
    ws, pk, x, _, a1, idx, dz, norm = c[:8]
    dz = dz if dz2 is None else dz2
    idx = idx if idx1 is None else idx1
    g = [torch.empty_like(ws[i]) for i in (2, 3, 0, 1)]
    C().cn_conv12_bwd(x[lo:hi].contiguous(), idx[lo:hi].contiguous(), a1[lo:hi].contiguous(),
                      dz[lo:hi].contiguous(), pk, *g, *norm)
    torch.cuda.synchronize()
    return g


def rel_norm(ref64, t):
    return float((ref64 - t.double()).norm() / ref64.norm())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("dead", [0, 1], ids=["live", "half_dead"])
@pytest.mark.parametrize("argmax", ARGMAX)
def test_against_dense_kernel_and_aten(B, argmax, dead):
    c = case(B, argmax, dead)
    g = backward(c, 0, B)
    sums = [torch.zeros_like(t, dtype=torch.float64) for t in g]
    for lo in range(0, B, CHUNK):
        for s, t in zip(sums, backward(c, lo, min(lo + CHUNK, B))):
            s += t.double()
    errs = [rel_norm(s, t) for s, t in zip(sums, g)]
    for name, err in zip(NAMES, errs):
        print(f"B={B} argmax={argmax} dead={dead} {name} {err:.3e}")
    aten = None
    if argmax == "random":
        ws, _, _, xn, a1, idx1, dz2 = c[:7]
        a1q = a1.permute(0, 3, 1, 2).float().requires_grad_()
        F.conv2d(a1q, bf(ws[2]), ws[3]).backward(dz2.float().permute(0, 3, 1, 2))
        da1_ref = bf(a1q.grad.permute(0, 2, 3, 1))
        dconv = bf(unpool2x2(da1_ref, conv1_codes(idx1) & 3, a1, 26)).permute(0, 3, 1, 2)
        w1q = ws[0].clone().requires_grad_()
        b1q = ws[1].clone().requires_grad_()
        F.conv2d(bf(xn), w1q, b1q, padding=1).backward(dconv)
        aten = (rel_err(g[2], w1q.grad), rel_err(g[3], b1q.grad))
        print(f"B={B} dead={dead} ATen dw1 {aten[0]:.3e} db1 {aten[1]:.3e}")
    for name, err in zip(NAMES, errs):
        assert err < (BOUND1 if name in ("dw1", "db1") else BOUND2), name
    if aten is not None:
        assert aten[0] < BOUND_ATEN and aten[1] < BOUND_ATEN


@pytest.mark.parametrize("B", BATCHES)
def test_all_windows_dead(B):
    c = case(B, "random", 2)
    # the live twin: this case's own a1 and dz2 with every window's code set
    live_codes = make_codes(c[8], torch.ones_like(c[9]))
    g_dead = backward(c, 0, B)
    g_live = backward(c, 0, B, idx1=live_codes)
    assert torch.equal(g_dead[2], torch.zeros_like(g_dead[2]))
    assert torch.equal(g_dead[3], torch.zeros_like(g_dead[3]))
    assert g_live[2].abs().max() > 0 and g_live[3].abs().max() > 0
    assert torch.equal(g_dead[0], g_live[0]) and torch.equal(g_dead[1], g_live[1])


@pytest.mark.parametrize("image", [0, 1, -1])
def test_one_image(image):
    """dz2 zero but for one image: a mis-routed value is an O(1) error, not one term in a million."""
    B = CHUNK + 1
    c = case(B, "random", 1)
    i = image % B
    dz2 = torch.zeros_like(c[6])
    dz2[i] = c[6][i]
    g = backward(c, 0, B, dz2=dz2)
    r = backward(c, i, i + 1)  # the 4-wave kernel on that image alone
    errs = [rel_norm(r[k].double(), g[k]) for k in (2, 3)]
    print(f"image {i} dw1 {errs[0]:.3e} db1 {errs[1]:.3e}")
    assert errs[0] < BOUND1 and errs[1] < BOUND1


def test_deterministic():
    c = case(2300, "random", 1)
    for name, a, b in zip(NAMES, backward(c, 0, 2300), backward(c, 0, 2300)):
        assert torch.equal(a, b), name
