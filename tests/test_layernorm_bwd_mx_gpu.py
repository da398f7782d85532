"""The MXFP8-writing LayerNorm backward (layernorm_bwd_mx): dx against layernorm_bwd's bits and fp64, its bytes
against the quantiser's on that dx, its band column sums, and the Functions with the fused path on and off."""
import pytest
import torch

from test_mxfp8_gpu import C, mx_ref, mx_ref_t
from vit_rows_common import F32, F64, check_colsum, check_ln_bwd, ln_bwd_case, ln_xhat

pytestmark = pytest.mark.gpu

# layernorm_fwd_mx's shapes: one row; a second band of one row, q with column padding; D no multiple of 64 or 128 and
# bands of pure row padding; the ViT width (two vectors per lane); the largest D and image
SHAPES = [(1, 32), (33, 64), (130, 160), (257, 768), (64, 2048)]


def _run(c, colwise=True):
    """(dx, q, s, qt, st, cs_part, dw, db) of layernorm_bwd_mx and layernorm_bwd's (dx, dw, db) on the case c."""
    x, w, b, dy = c["x"].cuda(), c["w"].cuda(), c["b"].cuda(), c["dy"].cuda()
    dres = None if c["dres"] is None else c["dres"].cuda()
    _, stats = C().layernorm_fwd(x, w, b, c["eps"])
    dw, db, dw0, db0 = (torch.full_like(w, float("nan")) for _ in range(4))
    out = C().layernorm_bwd_mx(dy, x, stats, w, dres, dw, db, colwise)
    return (*out, dw, db), (C().layernorm_bwd(dy, x, stats, w, dres, dw0, db0), dw0, db0)


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("rows,D", SHAPES)
def test_bytes_and_values(rows, D, with_dres):
    c = ln_bwd_case(rows, D, with_dres)
    (dx, q, s, qt, st, cs, dw, db), (dx0, _, _) = _run(c)
    Rp, Cp, nb = (rows + 127) // 128 * 128, (D + 127) // 128 * 128, (rows + 31) // 32
    assert torch.equal(dx, dx0)
    assert q.shape == (rows, Cp) and s.shape == (rows, Cp // 32) and qt.shape == (D, Rp) and st.shape == (D, Rp // 32)
    for got, want in zip((q, s, qt, st), C().mx_quantize(dx, True, True)):
        assert torch.equal(got, want)
    for got, want in zip((q, s, qt, st), mx_ref(dx)[:2] + mx_ref_t(dx)[:2]):  # full padded shapes
        assert torch.equal(got.cpu(), want)
    assert not q[:, D:].any() and not qt[:, rows:].any()
    assert bool((s[:, D // 32:] == 127).all()) and bool((st[:, nb:] == 127).all())
    assert not any(bool((t == 255).any()) for t in (s, st))
    check_ln_bwd(dx.cpu(), dw.cpu(), db.cpu(), c, f"layernorm_bwd_mx rows={rows} D={D} dres={with_dres}")
    assert cs.dtype == torch.float32 and cs.shape == (nb, D)
    check_colsum(cs.to(F64).sum(0).cpu(), dx.cpu())
    for k in range(nb):  # each band's sums are those of its own rows
        check_colsum(cs[k].to(F64).cpu(), dx[32 * k:32 * k + 32].cpu(), f"band {k}")
    (dx_r, q_r, s_r, qt_r, st_r, cs_r, dw_r, db_r), _ = _run(c, colwise=False)
    assert qt_r is None and st_r is None and cs_r is None
    for got, want in zip((dx_r, q_r, s_r, dw_r, db_r), (dx, q, s, dw, db)):
        assert torch.equal(got, want)


def test_many_bands():
    """32801 rows = 1026 bands, past reduce_parts' first level; dy lives in rows 0, 31, 32 and 32800 only, so a row or
    band lost or counted twice is a quarter of dw / db."""
    rows, D, live = 32801, 32, (0, 31, 32, 32800)
    c = ln_bwd_case(rows, D, False)
    dy = torch.zeros_like(c["dy"])
    dy[list(live)] = c["dy"][list(live)]
    c["dy"] = dy
    (dx, q, s, qt, st, cs, dw, db), (dx0, _, _) = _run(c)
    assert torch.equal(dx, dx0)
    check_ln_bwd(dx.cpu(), dw.cpu(), db.cpu(), c, "layernorm_bwd_mx rows=32801 D=32")
    bands = sorted({r // 32 for r in live})
    hit = (st != 127).any(0).cpu()
    assert hit.nonzero().flatten().tolist() == bands


@pytest.mark.parametrize("D,dt", [(48, torch.bfloat16), (4096, torch.bfloat16), (64, torch.float32)])
def test_refuses_bad_shapes(D, dt):
    x = torch.zeros(4, D, device="cuda", dtype=torch.bfloat16)
    f = [torch.zeros(D, device="cuda") for _ in range(3)]
    with pytest.raises(RuntimeError):
        C().layernorm_bwd_mx(x.to(dt), x, torch.zeros(4, 2, device="cuda"), f[0], None, f[1], f[2], True)


def _count(monkeypatch, T, name, calls):
    """Counts the calls of the extension's ``name`` made from ringdp.ops.transformer into calls[name]."""
    fn = getattr(T.C, name)
    monkeypatch.setattr(T.C, name, lambda *a: (calls.__setitem__(name, calls.get(name, 0) + 1), fn(*a))[1])


@pytest.mark.parametrize("ln_first", [True, False])
def test_second_consumer_of_the_linear_output(monkeypatch, ln_first):
    """z = LN(x1) + 5 x1 (either order): autograd may add the second gradient into the LayerNorm's dx in place, which
    keeps its attributes; the linear must then quantise the sum itself, as with the knob off."""
    from ringdp.ops import transformer as T

    M, D = 130, 128
    g = torch.Generator().manual_seed(5)
    a0, dy = (torch.randn(M, D, generator=g).bfloat16().cuda() for _ in range(2))
    ln = torch.nn.LayerNorm(D, eps=1e-6).cuda()
    wp, bp = ((torch.randn(*sh, generator=g) / 8).cuda().requires_grad_() for sh in ((D, D), (D,)))

    def run(fused):
        monkeypatch.setattr(T, "_MX_LN_BWD_FUSED", fused)
        a = a0.clone().requires_grad_()
        wp.grad = bp.grad = None
        x1 = T.LinearF.apply(a, wp, bp, None, 0, False)
        norm = lambda: T.LayerNormF.apply(x1, ln.weight, ln.bias, ln.eps)  # (node order = evaluation order)
        (norm() + 5 * x1 if ln_first else 5 * x1 + norm()).backward(dy)
        return a.grad, wp.grad.clone(), bp.grad.clone()

    T.set_fp8(True, recipe="mx")
    try:
        want, got = run(False), run(True)
    finally:
        T.set_fp8(False)
    for a, e in zip(got, want):
        assert torch.equal(a, e)


def test_functions_match_unfused(monkeypatch):
    """proj (+ residual) -> ln_2 fork -> MLP (+ residual) -> final LayerNorm: both LayerNorm backwards hand their dx
    to an MXFP8 linear.  dx is bit-equal and the MXFP8 bytes byte-equal, so everything but the two bias gradients
    (another summation order) is equal between the fused path and the quantiser passes."""
    from ringdp.ops import transformer as T

    M, D, Hd = 130, 128, 160
    g = torch.Generator().manual_seed(11)
    rnd = lambda *sh: torch.randn(*sh, generator=g)
    o, x0, dy = (rnd(M, D).bfloat16().cuda() for _ in range(3))
    lns = [torch.nn.LayerNorm(D, eps=1e-6).cuda() for _ in range(2)]
    with torch.no_grad():
        for ln in lns:
            ln.weight.copy_(1 + 0.25 * rnd(D))
            ln.bias.copy_(0.25 * rnd(D))
    wp, bp, w1, b1, w2, b2 = ((rnd(*sh) / 8).cuda().requires_grad_()
                              for sh in ((D, D), (D,), (Hd, D), (Hd,), (D, Hd), (D,)))
    params = [wp, bp, w1, b1, w2, b2] + [p for ln in lns for p in (ln.weight, ln.bias)]

    def run(fused):
        monkeypatch.setattr(T, "_MX_LN_BWD_FUSED", fused)
        a, r = o.clone().requires_grad_(), x0.clone().requires_grad_()
        for p in params:
            p.grad = None
        seen = {}
        x1 = T.LinearF.apply(a, wp, bp, r, 0, False)
        h, xr = T.layernorm_fork(x1, lns[0], w1)
        x2 = T.MLPMX.apply(h, w1, b1, w2, b2, xr)
        y = T.LayerNormF.apply(x2, lns[1].weight, lns[1].bias, lns[1].eps)
        if not fused:  # dz of proj and fc2, ln_2's dy (a hook would strip the fused run's attributes)
            for name, t in (("dz1", x1), ("dh", h), ("dz2", x2)):
                t.register_hook(lambda gr, name=name: seen.__setitem__(name, gr.detach().double().cpu()))
            seen.update(x1=x1.detach().cpu(), x2=x2.detach().cpu())
        y.backward(dy)
        return [y.detach(), a.grad, r.grad] + [p.grad.clone() for p in params], seen

    calls = {}
    for name in ("layernorm_bwd_mx", "mx_quantize", "colsum_f32"):
        _count(monkeypatch, T, name, calls)
    T.set_fp8(True, recipe="mx")
    try:
        want, seen = run(False)
        off = dict(calls)
        calls.clear()
        got, _ = run(True)
    finally:
        T.set_fp8(False)
    # the fused path is taken: both LayerNorm backwards, and neither linear quantises or column-sums its dz
    assert "layernorm_bwd_mx" not in off and calls["layernorm_bwd_mx"] == 2
    assert calls["mx_quantize"] == off["mx_quantize"] - 2 and calls.get("colsum_f32", 0) == off["colsum_f32"] - 2
    n = 2 * (M + 8) * 2.0 ** -24
    tol = {4: n * seen["dz1"].abs().sum(0), 8: n * seen["dz2"].abs().sum(0)}  # bp, b2: another summation order
    for i, g, x in ((9, seen["dh"].abs(), seen["x1"]), (11, dy.double().abs().cpu(), seen["x2"])):
        # LayerNorm weight / bias gradients (per-band partials of another split): twice check_ln_bwd's bounds
        xh = ln_xhat(x, 1e-6)
        exh = float((ln_xhat(x, 1e-6, F32).to(F64) - xh).abs().max())
        tol[i], tol[i + 1] = n * (g * xh.abs()).sum(0) + 16 * exh * g.sum(0), n * g.sum(0)
    for i, (a, e) in enumerate(zip(got, want)):
        if i in tol:
            assert bool(((a.double() - e.double()).abs().cpu() <= tol[i]).all()), i
        else:
            assert torch.equal(a, e), i
