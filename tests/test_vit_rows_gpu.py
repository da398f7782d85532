"""The ViT row and layout kernels (``csrc/kernels/vit.hip``) against the float64 references of ``vit_rows_common``,
called directly at the smallest shapes that reach every code path: all LayerNorm vector widths and their dispatch
boundaries, ragged row counts, both softmax kernels, the grid-stride tails past the block caps, and the pads.
The tolerances are derived in ``vit_rows_common`` from the references alone; ``test_vit_rows_cpu.py`` shows that
they reject wrong formulas."""
import pytest
import torch

import vit_rows_common as vc
from vit_rows_common import F32, F64

pytestmark = pytest.mark.gpu


def C():
    import ringdp

    return ringdp._C


def cuda(*ts):
    return [t.cuda() if t is not None else None for t in ts]


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd(c):
    x, w, b = cuda(c["x"], c["w"], c["b"])
    y, stats = C().layernorm_fwd(x, w, b, c["eps"])
    assert stats.shape == (x.shape[0], 2)
    return y, stats


@pytest.mark.parametrize("D", vc.LN_DS)
def test_layernorm_fwd(D):
    cases = [vc.ln_fwd_case(rows, D) for rows in vc.LN_FWD_ROWS]
    if D == 768:
        cases.append(vc.ln_fwd_case(5, D, 1e-2))  # a dropped or misplaced eps shows here
    for c in cases:
        y, stats = _ln_fwd(c)
        stats = stats.cpu()
        vc.check_ln_fwd(y.cpu(), stats[:, 0], stats[:, 1], c, f"layernorm_fwd rows={c['x'].shape[0]} D={D} eps={c['eps']}")


def _ln_bwd_both(c):
    """dx, dw, db of layernorm_bwd after checking that layernorm_bwd_colsum returns the same bits and column sums
    that are those of its dx."""
    _, stats = _ln_fwd(c)
    x, w, dy, dres = cuda(c["x"], c["w"], c["dy"], c["dres"])
    D = x.shape[-1]
    dw0, db0, dw1, db1 = (torch.full((D,), float("nan"), device="cuda") for _ in range(4))
    dx0 = C().layernorm_bwd(dy, x, stats, w, dres, dw0, db0)
    dx1, part = C().layernorm_bwd_colsum(dy, x, stats, w, dres, dw1, db1)
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)
    assert part.dtype == F32 and part.shape[1] == D
    vc.check_colsum(part.to(F64).sum(0).cpu(), dx1.cpu())
    return dx0.cpu(), dw0.cpu(), db0.cpu()


@pytest.mark.parametrize("D", vc.LN_DS)
def test_layernorm_bwd(D):
    for rows in vc.LN_BWD_ROWS:
        for with_dres in (False, True):
            c = vc.ln_bwd_case(rows, D, with_dres)
            vc.check_ln_bwd(*_ln_bwd_both(c), c, f"layernorm_bwd rows={rows} D={D} dres={with_dres}")


def test_layernorm_bwd_past_the_block_cap():
    """16401 rows: 1024 blocks of 17 rows, the last 59 without any.  dy is planted in rows 0, 16, 17 and 16400
    only, so a row lost or counted twice at a block boundary is a quarter of dw / db."""
    c = vc.ln_bwd_tail_case()
    dx, dw, db = _ln_bwd_both(c)
    vc.check_ln_bwd(dx, dw, db, c, "layernorm_bwd rows=16401 D=64")
    dead = torch.ones(vc.LN_TAIL[0], dtype=torch.bool)
    dead[list(vc.LN_TAIL_LIVE)] = False
    assert float(dx[dead].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ e4m3 LayerNorm
@pytest.mark.parametrize("D", (128, 768, 1280, 2048))
def test_layernorm_fwd_q8(D):
    """The e4m3 LayerNorm writes layernorm_fwd's values, quantised with the delayed scale hist[0] / 448: q, its
    transpose, the scale, the stats and the per-block |y|max are all determined bit for bit.  D = 2048 takes
    131,328 B of dynamic LDS."""
    for rows in (16, 80, 192):  # 80: a 16-row last block
        g = torch.Generator().manual_seed(D + rows)
        x = (torch.randn(rows, D, generator=g) * 2 + 0.5).bfloat16().cuda()
        w, b = cuda(*vc.ln_params(D, rows))
        y, stats = C().layernorm_fwd(x, w, b, vc.LN_EPS)
        yf = y.float().cpu()  # the expected values are fp32 arithmetic on the CPU: true divisions, no reciprocals
        nblk = (rows + 63) // 64
        assert C().layernorm_q8_slots(rows) == nblk
        for frac in (1.0, 0.5):  # 0.5: the clamp at +-448 is used
            h0 = yf.abs().max().reshape(1) * frac
            hist = torch.zeros(1 + nblk, device="cuda")
            hist[:1] = h0.cuda()
            stats8, q, qt, scale = C().layernorm_fwd_q8(x, w, b, vc.LN_EPS, hist)
            what = f"layernorm_fwd_q8 rows={rows} D={D} amax x {frac}"
            assert torch.equal(stats8, stats), what
            hist = hist.cpu()
            assert torch.equal(hist[:1], h0), what
            want_scale = h0.clamp_min(1e-12) / 448.0
            assert torch.equal(scale.cpu(), want_scale), (what, scale, want_scale)
            # multiply by the fp32 reciprocal as the kernel does: x / s can differ from x * (1 / s) by one e4m3 ulp
            want = (yf * (1.0 / want_scale)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
            assert q.shape == (rows, D) and qt.shape == (D, rows) and q.dtype == torch.uint8
            if frac < 1:
                assert int((want.view(torch.float8_e4m3fn).float().abs() == 448).sum()) > 0
            bad = (q.cpu() != want).nonzero()
            assert bad.numel() == 0, (what, len(bad), bad[0].tolist(), int(q[tuple(bad[0])]), int(want[tuple(bad[0])]))
            assert torch.equal(qt, q.t()), what
            for blk in range(nblk):
                assert float(hist[1 + blk]) == float(yf[64 * blk:64 * blk + 64].abs().max()), (what, blk)


# ------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("T,Tp", vc.SM_SHAPES)
def test_softmax_fwd(T, Tp):
    s = vc.softmax_scores(T, Tp)  # NaN in padded key columns and query rows
    p = C().softmax_fwd(s.cuda(), T, vc.SM_SCALE)
    assert p.dtype == torch.bfloat16 and p.shape == s.shape
    vc.check_softmax_fwd(p.cpu(), s, T, f"softmax_fwd T={T} Tp={Tp}")


@pytest.mark.parametrize("T,Tp", vc.SM_SHAPES)
def test_softmax_bwd(T, Tp):
    p, dp = vc.softmax_bwd_inputs(T, Tp)
    ds = C().softmax_bwd(p.cuda(), dp.cuda(), T, vc.SM_SCALE)
    assert ds.dtype == torch.bfloat16 and ds.shape == p.shape
    vc.check_softmax_bwd(ds.cpu(), p, dp, T, f"softmax_bwd T={T} Tp={Tp}")


# ------------------------------------------------------------------------------------------------ GELU backward
@pytest.mark.parametrize("ones", [True, False], ids=["dy_one", "dy_randn"])
def test_gelu_bwd_every_finite_bf16(ones):
    pre = vc.all_finite_bf16()
    dy = vc.gelu_dy(pre.numel(), ones)
    dx = C().gelu_bwd(dy.cuda(), pre.cuda())
    vc.check_gelu_bwd(dx.cpu(), pre, dy)


def test_gelu_bwd_past_the_block_cap():
    n = 8 * (8192 * 256 + 300)  # 8192 blocks, then a grid-stride tail of 300 vectors
    g = torch.Generator().manual_seed(11)
    pre = (3 * torch.randn(n, generator=g)).bfloat16().cuda()
    dy = torch.randn(n, generator=g).bfloat16().cuda()
    dx = C().gelu_bwd(dy, pre)
    vc.check_gelu_bwd(dx, pre, dy, "gelu_bwd tail")  # the float64 reference is built on the GPU


# ------------------------------------------------------------------------------------------------ layouts
def _layouts(B, T, H, Dh, Tp, x, rows, split=True, heads=True):
    """x [B*T, 3*H*Dh], rows [B*T, H*Dh] on the GPU; the references run there too (pure view / permute / pad)."""
    if split:
        q, k, v = C().qkv_split(x, B, T, H, Tp)
        for got, want in zip((q, k, v), vc.qkv_split(x, B, T, H, Tp)):
            assert got.shape == (B * H, Tp, Dh) and torch.equal(got, want)
            assert T == Tp or float(got[:, T:].float().abs().max()) == 0.0
        assert torch.equal(C().qkv_merge(q, k, v, B, T), x)
        junk = [t.clone() for t in (q, k, v)]  # the merge must not read the padded rows
        for t in junk:
            t[:, T:] = float("nan")
        assert torch.equal(C().qkv_merge(*junk, B, T), vc.qkv_merge(q, k, v, B, T))
    if heads:
        o = C().rows_to_heads(rows, B, T, H, Tp)
        assert o.shape == (B * H, Tp, Dh) and torch.equal(o, vc.rows_to_heads(rows, B, T, H, Tp))
        assert T == Tp or float(o[:, T:].float().abs().max()) == 0.0
        o[:, T:] = float("nan")
        back = C().heads_to_rows(o, B, T)
        assert back.shape == rows.shape and torch.equal(back, rows)


@pytest.mark.parametrize("B,T,H,Dh,Tp", vc.LAYOUT_SHAPES)
def test_layout_kernels(B, T, H, Dh, Tp):
    _layouts(B, T, H, Dh, Tp, vc.distinct_bf16(B * T, 3 * H * Dh).cuda(), vc.distinct_bf16(B * T, H * Dh, seed=1).cuda())


def _randn_bf16(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(shape[0])).bfloat16().cuda()


def test_layout_kernels_past_the_block_cap():
    """(48, 197, 12, 64, 208): 11232 and 10638 blocks' worth of vectors for qkv_split and qkv_merge, against a cap
    of 8192.  The two head shuffles move a third of that and reach the cap only at ViT-B's batch 128 (14976 and
    9456 blocks' worth), so they get that batch."""
    B, T, H, Dh, Tp = vc.LAYOUT_TAIL
    _layouts(B, T, H, Dh, Tp, _randn_bf16(B * T, 3 * H * Dh), _randn_bf16(B * T, H * Dh))
    assert 3 * B * H * Tp * Dh // 8 > 8192 * 256 and B * T * 3 * H * Dh // 8 > 8192 * 256
    B = 128
    assert B * H * Tp * Dh // 8 > 8192 * 256 and B * T * H * Dh // 8 > 8192 * 256
    _layouts(B, T, H, Dh, Tp, None, _randn_bf16(B * T, H * Dh), split=False)


@pytest.mark.parametrize("B,T,D", vc.CLS_SHAPES)
def test_cls_rows(B, T, D):
    x = vc.distinct_bf16(B * T, D).cuda()
    y = C().cls_rows(x, B, T, False)
    assert y.shape == (B, D) and torch.equal(y, vc.cls_rows(x, B, T, False))
    back = C().cls_rows(y, B, T, True)
    assert back.shape == (B, T, D) and torch.equal(back, vc.cls_rows(y, B, T, True))


# ------------------------------------------------------------------------------------------------ tokens, patches
@pytest.mark.parametrize("B,NP,D", vc.ASSEMBLE_SHAPES + ((16, 196, 768),))  # the last: past the 8192-block cap
def test_assemble_tokens(B, NP, D):
    patches, cls, pos = vc.assemble_case(B, NP, D)
    out = C().assemble_tokens(*cuda(patches, cls, pos))
    want = vc.assemble(patches, cls, pos, F32).bfloat16()  # one fp32 add, one rounding: a single correct answer
    assert out.shape == want.shape and torch.equal(out.cpu(), want)


@pytest.mark.parametrize("B,NP,D", vc.ASSEMBLE_SHAPES)
def test_assemble_tokens_bwd(B, NP, D):
    T = NP + 1
    dout = torch.randn(B, T, D, generator=torch.Generator().manual_seed(B + NP)).bfloat16()
    dpos, dcls = torch.full((T * D,), float("nan"), device="cuda"), torch.full((D,), float("nan"), device="cuda")
    dpatches = C().assemble_tokens_bwd(dout.cuda(), dpos, dcls)
    want_dp, want_dpos, _ = vc.assemble_bwd(dout)
    assert dpatches.shape == (B, NP, D) and torch.equal(dpatches.cpu(), want_dp)
    vc.assert_sum_close(dpos.cpu().view(T, D), want_dpos, B, dout.to(F64).abs().sum(0), what="assemble_tokens_bwd dpos")
    assert torch.equal(dcls, dpos[:D])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,Cc,H,W,P", vc.PATCH_SHAPES + ((16, 3, 224, 224, 16),))  # the last: past the block cap
def test_patchify(B, Cc, H, W, P, bf16):
    x = vc.patch_images(B, Cc, H, W, bf16)
    out = C().patchify(x.cuda(), P)
    want = vc.patchify(x, P).bfloat16()  # unfold in fp32 on the CPU, one rounding
    assert out.dtype == torch.bfloat16 and out.shape == want.shape and torch.equal(out.cpu(), want)


# ------------------------------------------------------------------------------------------------ refusals
# Every call below is refused by a host-side check that runs before any allocation or launch (csrc/ops/nn_ops.cpp).
def _bf(*shape):
    return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)


def _f(*shape):
    return torch.zeros(*shape, device="cuda")


@pytest.mark.parametrize("op", ["layernorm_bwd", "layernorm_bwd_colsum"])
def test_layernorm_bwd_refuses_bad_shapes(op):
    f = getattr(C(), op)
    for D, wn, sn, dwn, dbn in ((12, 12, 8, 12, 12),    # D % 8 (the kernel reads 8-wide vectors)
                                (2056, 2056, 8, 2056, 2056),  # D > 2048 (red[4][2048])
                                (16, 8, 8, 16, 16), (16, 16, 6, 16, 16), (16, 16, 8, 8, 16), (16, 16, 8, 16, 8)):
        with pytest.raises(RuntimeError, match="layernorm backward"):
            f(_bf(4, D), _bf(4, D), _f(sn), _f(wn), None, _f(dwn), _f(dbn))


_BAD_LAYOUT_CALLS = {
    "qkv_split": [lambda: C().qkv_split(_bf(4, 48), 2, 2, 2, 1)],                                 # Tp < T
    "qkv_merge": [lambda: C().qkv_merge(_bf(3, 16, 8), _bf(3, 16, 8), _bf(3, 16, 8), 2, 4),       # B does not divide B*H
                  lambda: C().qkv_merge(_bf(4, 16, 8), _bf(4, 16, 8), _bf(2, 16, 8), 2, 4),       # dv smaller than dq
                  lambda: C().qkv_merge(_bf(4, 16, 12), _bf(4, 16, 12), _bf(4, 16, 12), 2, 4),    # Dh % 8
                  lambda: C().qkv_merge(_bf(4, 16, 8), _bf(4, 16, 8), _bf(4, 16, 8), 2, 17)],     # T > Tp
    "heads_to_rows": [lambda: C().heads_to_rows(_bf(4, 16, 8), 2, 17),                            # T > Tp
                      lambda: C().heads_to_rows(_bf(3, 16, 8), 2, 4),                             # B does not divide B*H
                      lambda: C().heads_to_rows(_bf(4, 16, 12), 2, 4)],                           # Dh % 8
    "rows_to_heads": [lambda: C().rows_to_heads(_bf(8, 24), 2, 4, 5, 16),                         # H does not divide D
                      lambda: C().rows_to_heads(_bf(8, 24), 2, 4, 2, 16),                         # Dh = 12
                      lambda: C().rows_to_heads(_bf(6, 16), 2, 4, 2, 16),                         # fewer rows than B*T
                      lambda: C().rows_to_heads(_bf(8, 16), 2, 4, 2, 3)],                         # Tp < T
}


@pytest.mark.parametrize("op", sorted(_BAD_LAYOUT_CALLS))
def test_layout_op_refuses_bad_shapes(op):
    for call in _BAD_LAYOUT_CALLS[op]:
        with pytest.raises(RuntimeError, match=op):
            call()


def test_cls_rows_refuses_bad_shapes():
    with pytest.raises(RuntimeError, match="cls_rows"):
        C().cls_rows(_bf(7, 8), 2, 4, False)
    with pytest.raises(RuntimeError, match="cls_rows"):
        C().cls_rows(_bf(8, 8), 2, 4, True)             # the reverse takes [B, D]


def test_assemble_tokens_bwd_refuses_bad_shapes():
    with pytest.raises(RuntimeError, match="assemble_tokens_bwd"):
        C().assemble_tokens_bwd(_bf(2, 3, 8), _f(16), _f(8))   # dpos smaller than T*D
    with pytest.raises(RuntimeError, match="assemble_tokens_bwd"):
        C().assemble_tokens_bwd(_bf(2, 3, 8), _f(24), _f(4))
    with pytest.raises(RuntimeError, match="assemble_tokens_bwd"):
        C().assemble_tokens_bwd(_bf(2, 1, 8), _f(8), _f(8))    # T = 1: no patch rows


def test_softmax_fwd_refuses_bad_shapes():
    with pytest.raises(RuntimeError, match="softmax_fwd"):
        C().softmax_fwd(_f(2, 16, 16), 17, 0.125)       # T > Tp
    with pytest.raises(RuntimeError, match="softmax_fwd"):
        C().softmax_fwd(_f(2, 16, 16), 0, 0.125)
    with pytest.raises(RuntimeError, match="softmax_fwd"):
        C().softmax_fwd(_f(2, 12, 16), 8, 0.125)        # rows are not whole [Tp, Tp] heads


def test_softmax_bwd_refuses_bad_shapes():
    with pytest.raises(RuntimeError, match="softmax_bwd"):
        C().softmax_bwd(_bf(2, 16, 16), _f(1, 16, 16), 8, 0.125)   # dp smaller than p
    with pytest.raises(RuntimeError, match="softmax_bwd"):
        C().softmax_bwd(_bf(2, 16, 16), _f(2, 16, 16), 17, 0.125)
    with pytest.raises(RuntimeError, match="softmax_bwd"):
        C().softmax_bwd(_bf(2, 12, 16), _f(2, 12, 16), 8, 0.125)   # rows are not whole [Tp, Tp] heads
