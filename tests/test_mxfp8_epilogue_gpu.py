"""The MXFP8-writing GEMM epilogue (gemm_mxfp8_quant_out): its bytes against the quantiser's on the bf16 output of
the same GEMM, the GELU-backward form and its column sums against fp64, and MLPMX against the fp64 emulation."""
import math

import pytest
import torch

from test_mxfp8_gpu import C, _operand, dequant, mx_ref, mx_ref_t, rel

pytestmark = pytest.mark.gpu

# one partial tile with 96 padding columns; two rows spilling into the second wave tile; two tiles each way with a
# wave tile of pure column padding (columns 320..383) and one beyond Mp = 384 that must stay unwritten
SHAPES = [(48, 32, 128), (130, 96, 192), (384, 320, 768)]


def _operands(M, N, K):
    """MXFP8 A [M, K], B [N, K] with products of O(1): _operand's row / k-block steps, A scaled down by the
    largest product."""
    a, b = _operand(M, K, 1), _operand(N, K, 2)
    scale = float((a.double() @ b.double().t()).abs().max())
    aq, sa, _, _ = C().mx_quantize((a.float() / scale).bfloat16(), True, False)
    bq, sb, _, _ = C().mx_quantize(b, True, False)
    return aq, sa, bq, sb, aq.shape[1]


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_epilogue_bytes_match_quantiser(M, N, K, act):
    aq, sa, bq, sb, Kp = _operands(M, N, K)
    bias = pre = pre2 = None
    if act == 2:
        bias = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
        bias[:32] = -100.0  # GELU gives exact zeros: all-zero blocks in both orientations
        pre = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        pre2 = torch.empty_like(pre)
    y = C().gemm_mxfp8(aq, sa, bq, sb, M, N, Kp, True, bias, act, None, pre)
    q, s, qt, st = C().gemm_mxfp8_quant_out(aq, sa, bq, sb, M, N, Kp, bias, act, pre2)
    Mp, Np = (M + 127) // 128 * 128, (N + 127) // 128 * 128
    assert q.shape == (M, Np) and s.shape == (M, Np // 32) and qt.shape == (N, Mp) and st.shape == (N, Mp // 32)
    if act == 2:
        assert torch.equal(pre2, pre)
        assert float(y[:, :32].abs().max()) == 0.0 and (N == 32 or float(y[:, 32:].abs().max()) > 0.1)
    for got, want in zip((q, s, qt, st), mx_ref(y)[:2] + mx_ref_t(y)[:2]):  # full padded shapes
        assert torch.equal(got.cpu(), want)
    for got, want in zip((q, s, qt, st), C().mx_quantize(y, True, True)):
        assert torch.equal(got, want)
    assert not q[:, N:].any() and not qt[:, M:].any()
    assert bool((s[:, N // 32:] == 127).all()) and bool((st[:, (M + 31) // 32:] == 127).all())
    assert not any(bool((t == 255).any()) for t in (q, s, qt, st))


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_epilogue_gelu_backward_and_colsum(M, N, K):
    """act 3 has no bf16 comparator (gemm_mxfp8 rejects it): fp64 reference with the exact erf form.  Per block,
    |deq - v| <= amax_block / 14 (the worst e4m3 half-ulp over the lower edge of the scaled amax range, 16/224 =
    8/112) + 2e-2 max|v| (test_gemm_mxfp8's bf16-output tolerance); column sums of M bf16-rounded terms within
    M 2^-8 max|v| (factor 2 for the fp32 accumulation and the erf approximation)."""
    aq, sa, bq, sb, Kp = _operands(M, N, K)
    pre = (2 * torch.randn(M, N, generator=torch.Generator().manual_seed(4))).bfloat16().cuda()
    colsum = torch.empty(N, device="cuda")
    q, s, qt, st = C().gemm_mxfp8_quant_out(aq, sa, bq, sb, M, N, Kp, None, 3, pre, colsum)
    x = pre.cpu().double()
    grad = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    v = dequant(aq, sa, M, Kp) @ dequant(bq, sb, N, Kp).t() * grad
    vmax = float(v.abs().max())
    for name, got, ref in (("row", dequant(q, s, M, N), v), ("col", dequant(qt, st, N, M), v.t())):
        R, Cc = ref.shape
        pad = torch.zeros(R, (Cc + 31) // 32 * 32, dtype=torch.float64)
        pad[:, :Cc] = ref
        bound = pad.view(R, -1, 32).abs().amax(-1).repeat_interleave(32, 1)[:, :Cc] / 14 + 2e-2 * vmax
        err = (got - ref).abs()
        print(name, "max err / bound", float((err / bound).max()), "rel", rel(got, ref))
        assert bool((err <= bound).all())
    assert not any(bool((t == 255).any()) for t in (q, s, qt, st))
    cerr = float((colsum.cpu().double() - v.sum(0)).abs().max())
    print("colsum err", cerr, "bound", M * 2.0 ** -8 * vmax)
    assert cerr <= M * 2.0 ** -8 * vmax


def test_mlp_mx_matches_fp64_emulation():
    from ringdp.ops.transformer import MLPMX, mx_mlp_fusable, set_fp8

    M, D, Hd = 130, 128, 160
    g = torch.Generator().manual_seed(11)
    h = torch.randn(M, D, generator=g).bfloat16().cuda().requires_grad_()
    res = torch.randn(M, D, generator=g).bfloat16().cuda().requires_grad_()
    w1 = (torch.randn(Hd, D, generator=g) / 8).cuda().requires_grad_()
    b1 = torch.randn(Hd, generator=g).cuda().requires_grad_()
    w2 = (torch.randn(D, Hd, generator=g) / 8).cuda().requires_grad_()
    b2 = torch.randn(D, generator=g).cuda().requires_grad_()
    dy = torch.randn(M, D, generator=g).bfloat16().cuda()
    set_fp8(True, recipe="mx")
    try:
        assert mx_mlp_fusable(M, D, Hd) and not mx_mlp_fusable(M, 64, 128)
        y = MLPMX.apply(h, w1, b1, w2, b2, res)
        y.backward(dy)
    finally:
        set_fp8(False)
    assert not mx_mlp_fusable(M, D, Hd)  # the recipe is off again
    # References from what the Function quantised.  The activation's bytes are the quantiser's of gemm_mxfp8's bf16
    # output (shown byte for byte above); dz1 exists only as the epilogue's MXFP8 bytes, so those are taken from the
    # same call on the same operands (checked against fp64 above), and its bf16 values - which the column sums add
    # up - row by row: the column sums of a one-row call are that row.
    hq, hs, _, _ = C().mx_quantize(h.detach(), True, False)
    w1q, w1s, _, _ = C().mx_quantize(w1.detach(), True, False)
    pre = torch.empty(M, Hd, device="cuda", dtype=torch.bfloat16)
    a = C().gemm_mxfp8(hq, hs, w1q, w1s, M, Hd, hq.shape[1], True, b1.detach(), 2, None, pre)
    z1 = mx_ref(h)[2] @ mx_ref(w1)[2].t() + b1.detach().cpu().double()
    assert rel(pre.cpu(), z1) < 1e-2
    want_y = mx_ref(a)[2] @ mx_ref(w2)[2].t() + b2.detach().cpu().double() + res.detach().cpu().double()
    dyq, dys, _, _ = C().mx_quantize(dy, True, False)
    _, _, w2qt, w2st = C().mx_quantize(w2.detach(), False, True)
    dzq, dzs, dzqt, dzst = C().gemm_mxfp8_quant_out(dyq, dys, w2qt, w2st, M, Hd, dyq.shape[1], None, 3, pre)
    dz = torch.empty(M, Hd, device="cuda")
    for m in range(M):
        C().gemm_mxfp8_quant_out(dyq[m:m + 1], dys[m:m + 1], w2qt, w2st, 1, Hd, dyq.shape[1], None, 3, pre[m:m + 1], dz[m])
    assert torch.equal(dz.bfloat16().float(), dz) and rel(dequant(dzq, dzs, M, Hd), dz.cpu()) < 1 / 14
    dh = dequant(dzq, dzs, M, Hd) @ mx_ref_t(w1)[2].t()
    dw1 = dequant(dzqt, dzst, Hd, M) @ mx_ref_t(h)[2].t()
    dw2 = mx_ref_t(dy)[2] @ mx_ref_t(a)[2].t()
    print("y", rel(y.cpu(), want_y), "dh", rel(h.grad.cpu(), dh), "dw1", rel(w1.grad.cpu(), dw1), "dw2",
          rel(w2.grad.cpu(), dw2))
    assert rel(y.cpu(), want_y) < 1e-2
    assert rel(h.grad.cpu(), dh) < 1e-2
    assert rel(w2.grad.cpu(), dw2) < 1e-4
    assert rel(w1.grad.cpu(), dw1) < 1e-4
    assert torch.equal(res.grad, dy)
    torch.testing.assert_close(b2.grad.cpu().double(), dy.cpu().double().sum(0), atol=1e-3, rtol=1e-4)
    torch.testing.assert_close(b1.grad.cpu().double(), dz.cpu().double().sum(0), atol=1e-3, rtol=1e-4)
