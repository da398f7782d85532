"""The comparators of ``vit_rows_common`` must have teeth: on every input the GPU tests use, the fp32 emulation (the
reference formula in torch fp32, rounded to bf16) passes, and each plausible kernel mistake fails on at least one of
those inputs.  No GPU: the kernels themselves are run by ``test_vit_rows_gpu.py``."""
import math

import pytest
import torch
import torch.nn.functional as F

import vit_rows_common as vc
from vit_rows_common import F32, F64, bf16r

LN_FWD_CASES = [vc.ln_fwd_case(rows, D) for D in vc.LN_DS for rows in vc.LN_FWD_ROWS] + [vc.ln_fwd_case(5, 768, 1e-2)]
LN_BWD_CASES = [vc.ln_bwd_case(rows, D, dres) for D in vc.LN_DS for rows in vc.LN_BWD_ROWS for dres in (False, True)]


def rejected(check, cases):
    """The cases (by index) on which ``check`` raises."""
    bad = []
    for i, c in enumerate(cases):
        try:
            check(c)
        except AssertionError:
            bad.append(i)
    return bad


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd_variant(c, eps=None, denom=None, naive_var=False):
    x = c["x"].to(F32)
    D = x.shape[-1]
    eps = c["eps"] if eps is None else eps
    mean = x.sum(-1, keepdim=True) / (denom or D)
    var = (x * x).sum(-1, keepdim=True) / D - mean * mean if naive_var else ((x - mean) ** 2).sum(-1, keepdim=True) / (denom or D)
    rstd = 1.0 / torch.sqrt(var + eps)
    return bf16r((x - mean) * rstd * c["w"] + c["b"]), mean[:, 0], rstd[:, 0]


def test_layernorm_fwd_emulation_passes():
    for c in LN_FWD_CASES:
        y, m, r = vc.ln_fwd(c["x"], c["w"], c["b"], c["eps"], F32)
        vc.check_ln_fwd(bf16r(y), m, r, c)
        vc.check_ln_fwd(*_ln_fwd_variant(c), c)  # the variant builder with nothing switched on is right, too


def test_layernorm_constant_rows_give_the_bias_exactly():
    c = vc.ln_fwd_case(33, 768)
    y64 = vc.ln_fwd(c["x"], c["w"], c["b"], c["eps"])[0]
    const = [(r + 33) % 6 in (3, 4) for r in range(33)]
    assert sum(const) >= 10 and torch.equal(y64[const], c["b"].to(F64).expand(sum(const), -1))


@pytest.mark.parametrize("kw", [dict(eps=0.0), dict(denom=-8), dict(naive_var=True)], ids=["no_eps", "D_minus_8", "naive_var"])
def test_layernorm_fwd_wrong_variants_fail(kw):
    def check(c):
        k = dict(kw)
        if "denom" in k:
            k["denom"] = c["x"].shape[-1] - 8
        vc.check_ln_fwd(*_ln_fwd_variant(c, **k), c)

    bad = rejected(check, LN_FWD_CASES)
    print(kw, "rejected on", len(bad), "of", len(LN_FWD_CASES))
    assert bad
    if "eps" in kw:  # the eps = 1e-2 case is there for this
        assert len(LN_FWD_CASES) - 1 in bad


def test_layernorm_fwd_rows_are_checked_one_by_one():
    """One wrong row among 33 (the neighbour's values), which a max-normalised measure would not see on a small row."""
    c = vc.ln_fwd_case(33, 192)
    y, m, r = vc.ln_fwd(c["x"], c["w"], c["b"], c["eps"], F32)
    y = bf16r(y)
    y[32] = y[26]
    with pytest.raises(AssertionError, match=r"worst at \(32, "):
        vc.check_ln_fwd(y, m, r, c)


def _ln_bwd_emul(c, drop_m2=False, drop_last=None):
    x, dy, w = c["x"], c["dy"], c["w"]
    mean, rstd = vc.ln_stats(x, c["eps"], F32)
    xh = (x.to(F32) - mean) * rstd
    g = dy.to(F32)
    gw = g * w
    m2 = 0.0 if drop_m2 else (gw * xh).mean(-1, keepdim=True)
    dx = rstd * (gw - gw.mean(-1, keepdim=True) - xh * m2)
    if c["dres"] is not None:
        dx = dx + c["dres"].to(F32)
    dw, db = (g * xh).sum(0), g.sum(0)
    if drop_last == "dw":
        dw = (g * xh)[:-1].sum(0)
    if drop_last == "db":
        db = g[:-1].sum(0)
    return bf16r(dx), dw, db


def test_layernorm_bwd_emulation_passes():
    for c in LN_BWD_CASES + [vc.ln_bwd_tail_case()]:
        vc.check_ln_bwd(*_ln_bwd_emul(c), c)


@pytest.mark.parametrize("kw", [dict(drop_m2=True), dict(drop_last="dw"), dict(drop_last="db")], ids=["no_m2", "dw_last_row", "db_last_row"])
def test_layernorm_bwd_wrong_variants_fail(kw):
    bad = rejected(lambda c: vc.check_ln_bwd(*_ln_bwd_emul(c, **kw), c), LN_BWD_CASES)
    print(kw, "rejected on", len(bad), "of", len(LN_BWD_CASES))
    if kw.get("drop_last") == "dw":  # the last of 17 rows is the all-zero row (xhat = 0): nothing to lose there
        bad += [i for i, c in enumerate(LN_BWD_CASES) if c["x"].shape[0] == 17]
    assert len(set(bad)) == len(LN_BWD_CASES)  # every row count, every D
    with pytest.raises(AssertionError):   # and the planted rows of the tail case: row 16400 is one of four
        c = vc.ln_bwd_tail_case()
        vc.check_ln_bwd(*_ln_bwd_emul(c, **kw), c)


def test_colsum_check_sees_one_lost_row():
    c = vc.ln_bwd_case(33, 768, True)
    dx = _ln_bwd_emul(c)[0]
    vc.check_colsum(dx.float().sum(0), dx)
    with pytest.raises(AssertionError):
        vc.check_colsum(dx[:-1].float().sum(0), dx)


# ------------------------------------------------------------------------------------------------ softmax
def _softmax_variant(s, T, scale=vc.SM_SCALE, extra_key=False):
    z = s[..., :T, :T].to(F32) * scale
    mx = z.amax(-1, keepdim=True)
    if extra_key:
        mx = mx.clamp_min(0.0)
    e = torch.exp(z - mx)
    den = e.sum(-1, keepdim=True) + (torch.exp(-mx) if extra_key else 0.0)
    p = torch.zeros(s.shape)
    p[..., :T, :T] = e / den
    return bf16r(p)


def test_softmax_emulation_passes():
    for T, Tp in vc.SM_SHAPES:
        s = vc.softmax_scores(T, Tp)
        vc.check_softmax_fwd(bf16r(vc.softmax_fwd(s, T, vc.SM_SCALE, F32)), s, T)
        vc.check_softmax_fwd(_softmax_variant(s, T), s, T)
        p, dp = vc.softmax_bwd_inputs(T, Tp)
        assert float(p[:, T:].abs().max() if T < Tp else 0) == 0 and float(p[:, :, T:].abs().max() if T < Tp else 0) == 0
        vc.check_softmax_bwd(bf16r(vc.softmax_bwd(p, dp, T, vc.SM_SCALE, F32)), p, dp, T)


@pytest.mark.parametrize("kw", [dict(extra_key=True), dict(scale=1.0)], ids=["extra_key", "no_scale"])
def test_softmax_wrong_variants_fail(kw):
    def check(shape):
        s = vc.softmax_scores(*shape)
        vc.check_softmax_fwd(_softmax_variant(s, shape[0], **kw), s, shape[0])

    bad = rejected(check, vc.SM_SHAPES)
    print(kw, "rejected on", [vc.SM_SHAPES[i] for i in bad])
    assert bad


def test_softmax_extra_key_needs_a_moderate_spread():
    """The trap: with scores spread over more than about 30 after scaling, one padded key with score 0 adds
    exp(-max) ~ 0 and no comparator can see it; the plain randn rows are what catches it."""
    T, Tp = 13, 16
    s = vc.softmax_scores(T, Tp)
    wide = [t for t in range(T) if (t + T) % 5 == 2]  # randn * 300 + 1e4
    p = _softmax_variant(s, T, extra_key=True)
    ok = _softmax_variant(s, T)
    assert wide and torch.equal(p[:, wide], ok[:, wide])
    with pytest.raises(AssertionError):
        vc.check_softmax_fwd(p, s, T)


def test_softmax_checks_pads_and_wrong_bwd():
    T, Tp = 13, 16
    s = vc.softmax_scores(T, Tp)
    p = _softmax_variant(s, T)
    p[1, 14, 3] = 1e-30
    with pytest.raises(AssertionError, match="padded query rows"):
        vc.check_softmax_fwd(p, s, T)
    p, dp = vc.softmax_bwd_inputs(T, Tp)
    ds = vc.softmax_bwd(p, dp, T, vc.SM_SCALE, F32)
    vc.check_softmax_bwd(bf16r(ds), p, dp, T)
    pl, dl = p[..., :T, :T].float(), dp[..., :T, :T]
    wrong = torch.zeros_like(ds)
    wrong[..., :T, :T] = vc.SM_SCALE * pl * (dl - (pl * dl)[..., :-1].sum(-1, keepdim=True))  # dot misses the last key
    with pytest.raises(AssertionError):
        vc.check_softmax_bwd(bf16r(wrong), p, dp, T)


# ------------------------------------------------------------------------------------------------ GELU backward
def test_all_finite_bf16():
    pre = vc.all_finite_bf16()
    assert pre.numel() == 65280 and pre.numel() % 8 == 0 and bool(torch.isfinite(pre.float()).all())
    assert pre.view(torch.int16).unique().numel() == 65280


@pytest.mark.parametrize("ones", [True, False])
def test_gelu_bwd_emulation_passes_and_tanh_form_fails(ones):
    pre = vc.all_finite_bf16()
    dy = vc.gelu_dy(pre.numel(), ones)
    vc.check_gelu_bwd(bf16r(vc.gelu_grad(pre, dy, F32)), pre, dy)
    x = pre.float()
    xs = x.clamp(-20, 20)  # beyond, the tanh form is 0 or 1 to every digit (and x^3 would overflow)
    k = math.sqrt(2.0 / math.pi)
    t = torch.tanh(k * (xs + 0.044715 * xs ** 3))
    tanh_form = bf16r(dy.float() * (0.5 * (1 + t) + 0.5 * xs * (1 - t * t) * k * (1 + 3 * 0.044715 * xs * xs)))
    with pytest.raises(AssertionError) as e:
        vc.check_gelu_bwd(tanh_form, pre, dy)
    print(e.value)
    n_bad = int(str(e.value).split(": ")[1].split(" of ")[0])
    assert 100 < n_bad < 1000, n_bad  # the two forms differ by up to 1e-3 around |x| ~ 2..4, and nowhere else
    if ones:  # the reference is aten's erf-form gradient, too
        x = pre.float().requires_grad_()
        F.gelu(x).backward(dy.float())
        vc.check_gelu_bwd(bf16r(x.grad), pre, dy)


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("B,T,H,Dh,Tp", vc.LAYOUT_SHAPES)
def test_layout_references(B, T, H, Dh, Tp):
    """The permute / pad references against index-by-index definitions."""
    x = vc.distinct_bf16(B * T, 3 * H * Dh)
    q, k, v = vc.qkv_split(x, B, T, H, Tp)
    assert q.shape == (B * H, Tp, Dh)
    for which, t in enumerate((q, k, v)):
        for b, h, tt in ((0, 0, 0), (B - 1, H - 1, T - 1), (B // 2, H // 2, T // 2)):
            assert torch.equal(t[b * H + h, tt], x[b * T + tt, (which * H + h) * Dh:(which * H + h + 1) * Dh])
        assert float(t[:, T:].float().abs().sum()) == 0
    assert torch.equal(vc.qkv_merge(q, k, v, B, T), x)
    rows = vc.distinct_bf16(B * T, H * Dh, seed=1)
    o = vc.rows_to_heads(rows, B, T, H, Tp)
    for b, h, tt in ((0, 0, 0), (B - 1, H - 1, T - 1)):
        assert torch.equal(o[b * H + h, tt], rows[b * T + tt, h * Dh:(h + 1) * Dh])
    assert float(o[:, T:].float().abs().sum()) == 0 and torch.equal(vc.heads_to_rows(o, B, T), rows)


def test_cls_rows_reference():
    for B, T, D in vc.CLS_SHAPES:
        x = vc.distinct_bf16(B * T, D)
        y = vc.cls_rows(x, B, T, False)
        assert all(torch.equal(y[b], x[b * T]) for b in range(B))
        back = vc.cls_rows(y, B, T, True)
        assert torch.equal(back[:, 0], y) and float(back[:, 1:].float().abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ tokens, patches
@pytest.mark.parametrize("B,NP,D", vc.ASSEMBLE_SHAPES)
def test_assemble_reference_and_shifted_pos(B, NP, D):
    patches, cls, pos = vc.assemble_case(B, NP, D)
    ref32 = vc.assemble(patches, cls, pos, F32)
    assert torch.equal(ref32[:, 0], (cls + pos[:D]).expand(B, D)) and torch.equal(ref32[-1, NP], patches[-1, NP - 1].float() + pos[NP * D:])
    ref64 = vc.assemble(patches, cls, pos)
    vc.assert_bf16_close(bf16r(ref32), ref64, 0.0)
    shifted = vc.assemble(patches, cls, pos.view(NP + 1, D).roll(1, 0).reshape(-1), F32)
    assert not torch.equal(bf16r(shifted), bf16r(ref32))
    with pytest.raises(AssertionError):
        vc.assert_bf16_close(bf16r(shifted), ref64, 0.0)
    dout = vc.distinct_bf16(B, NP + 1, D).float().clamp(-8, 8).bfloat16()
    dpatches, dpos, dcls = vc.assemble_bwd(dout)
    assert dpatches.shape == (B, NP, D) and torch.equal(dcls, dpos[0])
    vc.assert_sum_close(dout.float().sum(0), dpos, B, dout.to(F64).abs().sum(0))
    with pytest.raises(AssertionError):
        vc.assert_sum_close(dout[:, 1:].float().sum(0), dpos[:-1], B, dout[:, :-1].to(F64).abs().sum(0))


@pytest.mark.parametrize("B,C,H,W,P", vc.PATCH_SHAPES)
def test_patchify_reference_and_swapped_kernel_axes(B, C, H, W, P):
    x = vc.patch_images(B, C, H, W, False)
    ref = vc.patchify(x, P)
    gh, gw = H // P, W // P
    assert ref.shape == (B * gh * gw, C * P * P)
    by_hand = x.view(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * P * P)
    assert torch.equal(ref, by_hand)
    swapped = x.view(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 5, 3).reshape(B * gh * gw, C * P * P)
    assert P == 1 or not torch.equal(bf16r(swapped), bf16r(ref))
    assert torch.equal(vc.patchify(x.bfloat16(), P), bf16r(ref).float())
