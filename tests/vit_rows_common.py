"""float64 references, comparators and inputs for the ViT row and layout kernels (``csrc/kernels/vit.hip``), shared by
the CPU tests (which show that the comparators reject wrong formulas) and the GPU tests (which run the kernels).

Every reference is written from the mathematical definition, not from the kernel, and takes exactly what the kernel
consumes: bf16 activations and fp32 parameters, upcast.  ``dtype=torch.float32`` evaluates the same formula in fp32:
that is the "fp32 emulation" the tolerances are derived from, never a kernel result.

Tolerances (computed here from the reference alone):

* bf16 outputs, per element, not normalised by any maximum:
  ``|got - ref| <= 2^-8 |ref| (1 + 2^-10) + slack + 1e-37``.  ``2^-8 |ref|`` is the half-ulp bound of round-to-nearest
  bf16 (8 significant bits), ``2^-10`` of it covers few-ulp fp32 intrinsics (rsqrtf, __expf, erff), ``1e-37`` covers
  bf16 subnormals, and ``slack = 8 max|f32 - f64|`` is the fp32 evaluation noise of the value before rounding (the 8
  allows for another reduction order).  The maximum is taken per row: every row is a reduction of its own, and a
  case-wide maximum would let one ill-conditioned row (variance 0: rstd = 1000) excuse all the others.
* fp32 sums of ``n`` terms in some fixed order (dw, db, column sums, dpos, dcls): the order-free worst case
  ``|err| <= (n + 8) 2^-24 sum|terms|``.
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
F32 = torch.float32


# ------------------------------------------------------------------------------------------------ comparators
def fp32_slack(f32, f64):
    """8 max|f32 - f64| over the last dim (kept): fp32 evaluation noise of a row, from the reference formula alone."""
    return 8.0 * (f32.to(F64) - f64).abs().amax(-1, keepdim=True)


def bf16_tol(ref64, slack):
    return 2.0 ** -8 * ref64.abs() * (1 + 2.0 ** -10) + slack + 1e-37


def _worst(err, tol, got, ref, what):
    over = torch.where(err <= tol, torch.zeros_like(err), torch.maximum(err - tol, torch.full_like(err, 1e-300)))
    over = torch.where(torch.isnan(err) | torch.isnan(tol), torch.full_like(err, math.inf), over)  # NaN fails
    if float(over.max()) == 0.0:
        return
    i = int(over.flatten().argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)) if err.dim() else ()
    raise AssertionError(f"{what}: {int((over > 0).sum())} of {err.numel()} elements out of tolerance; worst at "
                         f"{idx}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} "
                         f"tol {float(tol.flatten()[i])!r}")


def assert_bf16_close(got, ref64, slack, what="bf16 output"):
    """Per-element comparison of a bf16 kernel output with its float64 reference (see the module docstring)."""
    assert got.dtype == torch.bfloat16 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    g = got.to(F64)
    tol = bf16_tol(ref64, slack).expand_as(ref64)
    _worst((g - ref64).abs(), tol, g, ref64, what)


def assert_sum_close(got, ref64, n, abs_terms_sum, extra=0.0, what="fp32 sum"):
    """fp32 sum of n terms against float64: |err| <= (n + 8) 2^-24 sum|terms| (+ extra)."""
    assert got.dtype == F32 and got.shape == ref64.shape, (what, got.dtype, got.shape, ref64.shape)
    g = got.to(F64)
    tol = ((n + 8) * 2.0 ** -24 * abs_terms_sum + extra).expand_as(ref64)
    _worst((g - ref64).abs(), tol, g, ref64, what)


def assert_close_abs(got, ref64, tol, what):
    g = got.to(F64)
    _worst((g - ref64).abs(), tol.expand_as(ref64), g, ref64, what)


def bf16r(t):
    """Round to bf16: what a kernel's store does to the fp32 value."""
    return t.to(F32).bfloat16()


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_stats(x, eps, dtype=F64):
    xd = x.to(dtype)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def ln_fwd(x, w, b, eps, dtype=F64):
    """y, mean [rows], rstd [rows]."""
    mean, rstd = ln_stats(x, eps, dtype)
    y = (x.to(dtype) - mean) * rstd * w.to(dtype) + b.to(dtype)
    return y, mean[..., 0], rstd[..., 0]


def ln_xhat(x, eps, dtype=F64):
    mean, rstd = ln_stats(x, eps, dtype)
    return (x.to(dtype) - mean) * rstd


def ln_bwd(dy, x, w, eps, dres=None, dtype=F64):
    """dx [rows, D] (+ dres), dw [D], db [D] of y = xhat * w + b."""
    _, rstd = ln_stats(x, eps, dtype)
    xh = ln_xhat(x, eps, dtype)
    g = dy.to(dtype)
    gw = g * w.to(dtype)
    dx = rstd * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(dtype)
    return dx, (g * xh).sum(0), g.sum(0)


LN_DS = (8, 192, 512, 520, 768, 1024, 1032, 1280, 2048)  # all three VPL instantiations, both sides of each boundary
LN_FWD_ROWS = (1, 3, 5, 33)                              # no multiple of 4: the early-exit waves run
LN_BWD_ROWS = (1, 17, 33)                                # 1, 2 and 3 blocks with ragged rows_per_block
LN_EPS = 1e-6


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ln_rows(rows, D, seed):
    """bf16 [rows, D] with the row kinds mixed: randn, mean >> std, large mean, all zero, constant 1.0, large scale."""
    g = _gen(seed)
    x = torch.randn(rows, D, generator=g)
    for r in range(rows):
        kind = (r + rows) % 6
        if kind == 1:
            x[r] = 8 + 0.05 * x[r]
        elif kind == 2:
            x[r] = 100 + x[r]
        elif kind == 3:
            x[r] = 0.0
        elif kind == 4:
            x[r] = 1.0
        elif kind == 5:
            x[r] = 1e4 * x[r]
    return x.bfloat16()


def ln_params(D, seed):
    g = _gen(seed + 1000)
    return torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)


def ln_fwd_case(rows, D, eps=LN_EPS):
    seed = 7 * D + rows
    w, b = ln_params(D, seed)
    return dict(x=ln_rows(rows, D, seed), w=w, b=b, eps=eps)


def ln_bwd_case(rows, D, with_dres, eps=LN_EPS):
    c = ln_fwd_case(rows, D, eps)
    g = _gen(13 * D + rows)
    c["dy"] = torch.randn(rows, D, generator=g).bfloat16()
    c["dres"] = torch.randn(rows, D, generator=g).bfloat16() if with_dres else None
    return c


LN_TAIL = (16401, 64)            # past the 1024-block cap: rows_per_block = 17, trailing blocks without rows
LN_TAIL_LIVE = (0, 16, 17, 16400)


def ln_bwd_tail_case():
    """dy is zero except LN_TAIL_LIVE, so one lost or doubled row shows in dw / db (the sum bound at this row count
    would hide it otherwise)."""
    rows, D = LN_TAIL
    g = _gen(99)
    x = torch.randn(rows, D, generator=g).bfloat16()
    dy = torch.zeros(rows, D)
    for r in LN_TAIL_LIVE:
        dy[r] = torch.randn(D, generator=g)
    w, b = ln_params(D, 99)
    return dict(x=x, w=w, b=b, eps=LN_EPS, dy=dy.bfloat16(), dres=None)


def check_ln_fwd(y, mean, rstd, c, what="layernorm_fwd"):
    x, w, b, eps = c["x"], c["w"], c["b"], c["eps"]
    D = x.shape[-1]
    y64, m64, r64 = ln_fwd(x, w, b, eps)
    y32, m32, r32 = ln_fwd(x, w, b, eps, F32)
    assert_bf16_close(y, y64, fp32_slack(y32, y64), what + " y")
    assert_close_abs(mean, m64, D * 2.0 ** -24 * x.to(F64).abs().mean(-1) + 8 * (m32.to(F64) - m64).abs(), what + " mean")
    assert_close_abs(rstd, r64, 2.0 ** -20 * r64 + 8 * (r32.to(F64) - r64).abs(), what + " rstd")


def check_ln_bwd(dx, dw, db, c, what="layernorm_bwd"):
    x, w, eps, dy, dres = c["x"], c["w"], c["eps"], c["dy"], c["dres"]
    rows = x.shape[0]
    dx64, dw64, db64 = ln_bwd(dy, x, w, eps, dres)
    dx32 = ln_bwd(dy, x, w, eps, dres, F32)[0]
    assert_bf16_close(dx, dx64, fp32_slack(dx32, dx64), what + " dx")
    xh64 = ln_xhat(x, eps)
    exh = float((ln_xhat(x, eps, F32).to(F64) - xh64).abs().max())
    g = dy.to(F64).abs()
    assert_sum_close(dw, dw64, rows, (g * xh64.abs()).sum(0), 8 * exh * g.sum(0), what + " dw")
    assert_sum_close(db, db64, rows, g.sum(0), 0.0, what + " db")


def check_colsum(cs_total, dx, what="layernorm_bwd_colsum"):
    """cs_total: the fp32 partial column sums, summed; dx: the bf16 dx the kernel returned."""
    d = dx.to(F64)
    _worst((cs_total.to(F64) - d.sum(0)).abs(), (dx.shape[0] + 8) * 2.0 ** -24 * d.abs().sum(0), cs_total.to(F64),
           d.sum(0), what)


# ------------------------------------------------------------------------------------------------ softmax
SM_SHAPES = ((1, 16), (16, 16), (13, 16), (193, 208), (197, 208), (253, 256), (256, 256), (257, 272), (272, 272),
             (577, 592))  # vector kernel up to Tp = 256, scalar beyond; T on and off multiples of 4 and 64; T == Tp
SM_HEADS, SM_SCALE = 3, 0.125


def softmax_fwd(s, T, scale, dtype=F64):
    """p [..., Tp, Tp]: softmax(scale * s) over the first T keys of the first T query rows, 0 elsewhere."""
    z = s[..., :T, :T].to(dtype) * scale
    e = torch.exp(z - z.amax(-1, keepdim=True))
    p = torch.zeros(s.shape, dtype=dtype)
    p[..., :T, :T] = e / e.sum(-1, keepdim=True)
    return p


def softmax_bwd(p, dp, T, scale, dtype=F64):
    """ds = scale * p * (dp - sum_j dp_j p_j) over the first T keys / query rows, 0 elsewhere."""
    pl, dl = p[..., :T, :T].to(dtype), dp[..., :T, :T].to(dtype)
    ds = torch.zeros(p.shape, dtype=dtype)
    ds[..., :T, :T] = scale * pl * (dl - (pl * dl).sum(-1, keepdim=True))
    return ds


def softmax_scores(T, Tp, pad=float("nan")):
    """fp32 [heads, Tp, Tp]; query row t of every head has kind t % 5: randn, randn * 30 (the moderate spread the
    extra-key variant needs is the plain randn row), randn * 300 + 1e4 (the max subtraction has to work), all
    equal, one-hot dominant.  Padded key columns and query rows hold ``pad``."""
    g = _gen(1000 * T + Tp)
    s = torch.randn(SM_HEADS, Tp, Tp, generator=g)
    for t in range(T):
        kind = (t + T) % 5
        if kind == 1:
            s[:, t] *= 30
        elif kind == 2:
            s[:, t] = s[:, t] * 300 + 1e4
        elif kind == 3:
            s[:, t] = 3.0
        elif kind == 4:
            s[:, t, (7 * t) % T] += 400.0
    s[:, T:, :] = pad
    s[:, :, T:] = pad
    return s


def softmax_bwd_inputs(T, Tp):
    """p = bf16(reference softmax) with zero pads (not a kernel's output); dp with NaN in padded key columns and a
    finite 1e30 in padded query rows, where p is 0."""
    p = softmax_fwd(softmax_scores(T, Tp), T, SM_SCALE).to(F32).bfloat16()
    dp = torch.randn(SM_HEADS, Tp, Tp, generator=_gen(2000 * T + Tp))
    dp[:, T:, :] = 1e30
    dp[:, :, T:] = float("nan")
    return p, dp


def _check_pads(out, T, what):
    assert torch.equal(out[..., T:, :].float(), torch.zeros_like(out[..., T:, :].float())), what + ": padded query rows"
    assert torch.equal(out[..., :, T:].float(), torch.zeros_like(out[..., :, T:].float())), what + ": padded keys"


def check_softmax_fwd(p, s, T, what="softmax_fwd"):
    _check_pads(p, T, what)
    p64, p32 = softmax_fwd(s, T, SM_SCALE), softmax_fwd(s, T, SM_SCALE, F32)
    assert_bf16_close(p[..., :T, :T], p64[..., :T, :T], fp32_slack(p32, p64)[..., :T, :], what)


def check_softmax_bwd(ds, p, dp, T, what="softmax_bwd"):
    _check_pads(ds, T, what)
    d64, d32 = softmax_bwd(p, dp, T, SM_SCALE), softmax_bwd(p, dp, T, SM_SCALE, F32)
    assert_bf16_close(ds[..., :T, :T], d64[..., :T, :T], fp32_slack(d32, d64)[..., :T, :], what)


# ------------------------------------------------------------------------------------------------ GELU backward
def gelu_grad(pre, dy, dtype=F64):
    """dy * d/dx [x Phi(x)] = dy * (Phi(x) + x phi(x)), the erf form."""
    x = pre.to(dtype)
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy.to(dtype) * (cdf + x * pdf)


def all_finite_bf16():
    """Every finite bf16 bit pattern: 65280 values, a multiple of 8."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return bits.to(torch.int16).view(torch.bfloat16)


def gelu_dy(n, ones):
    return torch.ones(n).bfloat16() if ones else (2 * torch.randn(n, generator=_gen(5))).bfloat16()


def check_gelu_bwd(dx, pre, dy, what="gelu_bwd"):
    """The absolute term is 2^-22 |dy| instead of a slack: in fp32, 1 + erf(x / sqrt 2) cancels for negative x
    whatever kernel computes it (one fp32 ulp of 1.0, halved by the 0.5, with room for the erf's own ulps)."""
    assert_bf16_close(dx, gelu_grad(pre, dy), 2.0 ** -22 * dy.to(F64).abs(), what)


# ------------------------------------------------------------------------------------------------ layouts
LAYOUT_SHAPES = ((1, 1, 1, 8, 16), (3, 17, 2, 64, 32), (2, 197, 3, 64, 208), (2, 16, 4, 32, 16))  # (B, T, H, Dh, Tp)
LAYOUT_TAIL = (48, 197, 12, 64, 208)  # past the 8192-block cap for qkv_split, qkv_merge and rows_to_heads


def qkv_split(x, B, T, H, Tp):
    """[B*T, 3*H*Dh] -> q, k, v [B*H, Tp, Dh], rows >= T zero."""
    Dh = x.shape[-1] // (3 * H)
    t = F.pad(x.view(B, T, 3, H, Dh).permute(2, 0, 3, 1, 4), (0, 0, 0, Tp - T))
    return tuple(t.reshape(3, B * H, Tp, Dh).contiguous())


def qkv_merge(q, k, v, B, T):
    BH, Tp, Dh = q.shape
    t = torch.stack((q, k, v)).view(3, B, BH // B, Tp, Dh)[:, :, :, :T]
    return t.permute(1, 3, 0, 2, 4).reshape(B * T, 3 * (BH // B) * Dh).contiguous()


def rows_to_heads(rows, B, T, H, Tp):
    Dh = rows.shape[-1] // H
    return F.pad(rows.view(B, T, H, Dh).permute(0, 2, 1, 3), (0, 0, 0, Tp - T)).reshape(B * H, Tp, Dh).contiguous()


def heads_to_rows(o, B, T):
    BH, Tp, Dh = o.shape
    return o.view(B, BH // B, Tp, Dh)[:, :, :T].permute(0, 2, 1, 3).reshape(B * T, (BH // B) * Dh).contiguous()


def distinct_bf16(*shape, seed=0):
    """bf16 values that differ between neighbours in every dim (a permutation of bit patterns of normal numbers), so
    a misplaced element cannot equal the right one by chance."""
    n = math.prod(shape)
    bits = (torch.randperm(n, generator=_gen(seed + n)) % 0x3F00 + 0x2000).to(torch.int16)  # 2^-63 .. 2^63, positive
    sign = (torch.arange(n) % 2).to(torch.int16) << 15
    return (bits | sign).view(torch.bfloat16).reshape(shape)


CLS_SHAPES = tuple((B, T, D) for B in (1, 5) for T in (1, 17) for D in (8, 192))


def cls_rows(x, B, T, reverse):
    D = x.shape[-1]
    if not reverse:
        return x.view(B, T, D)[:, 0].contiguous()
    y = torch.zeros(B, T, D, dtype=x.dtype, device=x.device)
    y[:, 0] = x
    return y


# ------------------------------------------------------------------------------------------------ tokens, patches
ASSEMBLE_SHAPES = ((1, 1, 8), (3, 4, 192), (2, 196, 768))  # (B, NP, D)


def assemble(patches, cls, pos, dtype=F64):
    """[B, 1 + NP, D] = concat(cls, patches) + pos, before the bf16 rounding.  In fp32 this is one add, whose
    rounding to bf16 has a single correct answer."""
    B, NP, D = patches.shape
    tok = torch.cat((cls.to(dtype).view(1, 1, D).expand(B, 1, D), patches.to(dtype)), 1)
    return tok + pos.to(dtype).view(1, NP + 1, D)


def assemble_bwd(dout):
    """dpatches (bf16, a copy), dpos [T, D] and dcls [D] (float64 sums over the batch)."""
    dpos = dout.to(F64).sum(0)
    return dout[:, 1:].contiguous(), dpos, dpos[0]


def assemble_case(B, NP, D):
    g = _gen(B * 31 + NP)
    # distinct per token: token t's values sit around 4 t, so a pos or patch row shifted by one token shows
    patches = (torch.randn(B, NP, D, generator=g) + 4 * torch.arange(1, NP + 1).view(1, NP, 1)).bfloat16()
    pos = torch.randn(NP + 1, D, generator=g) - 3 * torch.arange(NP + 1).view(NP + 1, 1)
    return patches, torch.randn(D, generator=g), pos.reshape(-1)


PATCH_SHAPES = ((2, 3, 32, 32, 4), (1, 3, 32, 48, 16), (3, 2, 8, 8, 2), (1, 8, 2, 2, 1))  # (B, C, H, W, P)


def patchify(x, P):
    """NCHW -> [B * NP, C*P*P] patch rows, columns in (c, kh, kw) order: the im2col of a stride-P PxP convolution."""
    return F.unfold(x.float(), P, stride=P).transpose(1, 2).reshape(-1, x.shape[1] * P * P)


def patch_images(B, C, H, W, bf16):
    x = torch.randn(B, C, H, W, generator=_gen(H * W + C))
    return x.bfloat16() if bf16 else x
