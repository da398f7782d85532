"""The MXFP8-writing LayerNorm forward (layernorm_fwd_mx): its bytes against the quantiser's on layernorm_fwd's
bf16 rows, its values against fp64, and LayerNormForkMX in front of LinearF / MLPMX against the unfused Functions."""
import pytest
import torch
import torch.nn.functional as F

from test_mxfp8_gpu import C, dequant, mx_ref, mx_ref_t, rel

pytestmark = pytest.mark.gpu

EPS = 1e-6
# one row (the rest of its column blocks is padding); a second band of one row, q with column padding; D no
# multiple of 64 or 128 and bands of pure row padding; the ViT width (two vectors per lane); the largest D and image
SHAPES = [(1, 32), (33, 64), (130, 160), (257, 768), (64, 2048)]


def _inputs(rows, D):
    """x with row offsets and power-of-two magnitude steps from row to row, one constant row (variance 0, y = b);
    w stepping by powers of two from one 32-column block to the next, the last block (of several) w = b = 0."""
    g = torch.Generator().manual_seed(1000 * rows + D)
    r, nb = torch.arange(rows), D // 32
    x = torch.randn(rows, D, generator=g) * torch.exp2((r % 7 - 3).float())[:, None] + (r % 5 - 2).float()[:, None]
    if rows > 2:
        x[2] = 1.5
    w = (1 + torch.rand(D, generator=g)) * torch.exp2((torch.arange(nb) % 6 - 3).float()).repeat_interleave(32)
    b = torch.randn(D, generator=g) * 0.25
    if nb > 1:
        w[-32:] = 0
        b[-32:] = 0
    return x.bfloat16().cuda(), w.cuda(), b.cuda()


@pytest.mark.parametrize("rows,D", SHAPES)
def test_bytes_match_layernorm_then_quantiser(rows, D):
    x, w, b = _inputs(rows, D)
    y, stats = C().layernorm_fwd(x, w, b, EPS)
    stats_mx, q, s, qt, st = C().layernorm_fwd_mx(x, w, b, EPS, True)
    Rp, Cp = (rows + 127) // 128 * 128, (D + 127) // 128 * 128
    assert q.shape == (rows, Cp) and s.shape == (rows, Cp // 32) and qt.shape == (D, Rp) and st.shape == (D, Rp // 32)
    assert torch.equal(stats_mx, stats)
    if rows > 2:
        assert torch.equal(y[2].float(), b.bfloat16().float())
    for got, want in zip((q, s, qt, st), C().mx_quantize(y, True, True)):
        assert torch.equal(got, want)
    for got, want in zip((q, s, qt, st), mx_ref(y)[:2] + mx_ref_t(y)[:2]):  # full padded shapes
        assert torch.equal(got.cpu(), want)
    assert not q[:, D:].any() and not qt[:, rows:].any()
    assert bool((s[:, D // 32:] == 127).all()) and bool((st[:, (rows + 31) // 32:] == 127).all())
    if D > 32:  # the w = b = 0 block: all-zero blocks both ways
        assert bool((s[:, D // 32 - 1] == 127).all()) and bool((st[-32:] == 127).all())
    assert not any(bool((t == 255).any()) for t in (q, s, qt, st))
    stats_r, q_r, s_r, none_qt, none_st = C().layernorm_fwd_mx(x, w, b, EPS, False)
    assert none_qt is None and none_st is None
    assert torch.equal(stats_r, stats) and torch.equal(q_r, q) and torch.equal(s_r, s)


@pytest.mark.parametrize("rows,D", SHAPES)
def test_values_against_fp64(rows, D):
    """Per element |deq - y| <= amax_block / 14 (the e4m3 half-ulp bound of test_epilogue_gelu_backward_and_colsum)
    + 2^-7 max|y| (four bf16 half-ulps of the stored value: the rounding to bf16, the fp32 statistics and the shift
    of a block's amax).  The largest err / bound ratio is printed."""
    x, w, b = _inputs(rows, D)
    _, q, s, qt, st = C().layernorm_fwd_mx(x, w, b, EPS, True)
    y = F.layer_norm(x.cpu().double(), (D,), w.cpu().double(), b.cpu().double(), EPS)
    ymax = float(y.abs().max())
    for name, got, ref in (("row", dequant(q, s, rows, D), y), ("col", dequant(qt, st, D, rows), y.t())):
        R, Cc = ref.shape
        pad = torch.zeros(R, (Cc + 31) // 32 * 32, dtype=torch.float64)
        pad[:, :Cc] = ref
        bound = pad.view(R, -1, 32).abs().amax(-1).repeat_interleave(32, 1)[:, :Cc] / 14 + 2.0 ** -7 * ymax
        err = (got - ref).abs()
        print(name, (rows, D), "max err / bound", float((err / bound).max()), "rel", rel(got, ref))
        assert bool((err <= bound).all())


@pytest.mark.parametrize("consumer", ["linear", "mlp"])
def test_fork_mx_matches_unfused_functions(consumer):
    from ringdp.ops import transformer as T

    M, D, Hd = 130, 128, 160
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(M, D, generator=g).bfloat16().cuda()
    ln = torch.nn.LayerNorm(D, eps=EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(1 + 0.25 * torch.randn(D, generator=g))
        ln.bias.copy_(0.25 * torch.randn(D, generator=g))
    w1 = (torch.randn(Hd, D, generator=g) / 8).cuda().requires_grad_()
    b1 = torch.randn(Hd, generator=g).cuda().requires_grad_()
    w2 = (torch.randn(D, Hd, generator=g) / 8).cuda().requires_grad_()
    b2 = torch.randn(D, generator=g).cuda().requires_grad_()
    params = [ln.weight, ln.bias, w1, b1] + ([w2, b2] if consumer == "mlp" else [])
    dy = torch.randn(M, D if consumer == "mlp" else Hd, generator=g).bfloat16().cuda()

    def run(fused):
        x = x0.clone().requires_grad_(torch.is_grad_enabled())
        if fused:
            h, xr = T.layernorm_fork(x, ln, w1)
            q, s, qt, st = h._ringdp_mx
            assert (qt is None) == (st is None) == (not torch.is_grad_enabled())
        else:
            h, xr = T.LayerNormFork.apply(x, ln.weight, ln.bias, ln.eps)
            assert getattr(h, "_ringdp_mx", None) is None
        if consumer == "mlp":
            y = T.MLPMX.apply(h, w1, b1, w2, b2, xr)
        else:
            y = T.LinearF.apply(h, w1, b1, None, 0, False)
        if not torch.is_grad_enabled():
            return [y]
        for p in params:
            p.grad = None
        y.backward(dy)
        return [y.detach(), x.grad] + [p.grad.clone() for p in params]

    T.set_fp8(True, recipe="mx")
    try:
        want, got = run(False), run(True)
        with torch.no_grad():
            got_ng = run(True)
    finally:
        T.set_fp8(False)
    assert len(got) == len(want) == 2 + len(params)
    for a, e in zip(got + got_ng, want + want[:1]):
        assert torch.equal(a, e)
