"""Dropout / stochastic depth on the GPU: the kernels bit for bit against the numpy Philox oracle
(``dropout_common``), the autograd Functions, the device-resident generator state (eager and replayed from a
hipGraph), and the ViT wiring against the fp64 / bf16-storage oracles of ``test_model_parity_gpu``."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_common as dc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _snap(seed, step):
    """A snapshot tensor as rng_tick would write it: (seed, step) as the int64 views of the u64 values."""
    s = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed, step)]
    return torch.tensor(s, dtype=torch.int64, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _mask(shape, thr, seed, step, site):
    n = int(np.prod(shape))
    return torch.from_numpy(dc.element_keep(n, thr, seed, step, site).reshape(shape)).to(DEV)


def _rand_bf16(shape, seed, lo=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if lo is None:
        return torch.randn(shape, device=DEV, generator=g).bfloat16()
    mag = torch.rand(shape, device=DEV, generator=g) * 1.5 + lo  # |value| in [0.5, 2]
    sign = torch.randint(0, 2, shape, device=DEV, generator=g) * 2 - 1
    return (mag * sign).bfloat16()


def _want_dropout(x, mask, scale):
    return torch.where(mask, (x.float() * float(scale)).bfloat16(), torch.zeros((), device=DEV, dtype=torch.bfloat16))


def _ulp_bf16(v):
    """One bf16 ulp at the magnitude of the fp64 values ``v`` (8 significand bits)."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("p", [0.1, 0.5, 1 - 2 ** -17])
@pytest.mark.parametrize("shape", [(1, 8), (394, 64), (1031, 776), (4099, 3072)])
def test_dropout_bitwise(shape, p):
    """(4099, 3072) has more vectors than the capped grid covers in one pass: the grid-stride tail."""
    from ringdp._native import C

    thr, scale = dc.quantize(p)
    x = _rand_bf16(shape, 1)
    for seed, step, site in ((1234, 1, 0), (2 ** 63 + 2 ** 40 + 7, 2 ** 32 + 5, 3)):
        y = C.dropout_bf16(x, _snap(seed, step), site, thr)
        mask = _mask(shape, thr, seed, step, site)
        want = _want_dropout(x, mask, scale)
        assert y.dtype == torch.bfloat16 and y.shape == x.shape
        assert torch.equal(_bits(y), _bits(want)), (seed, step, site, int((_bits(y) != _bits(want)).sum()))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", [(394, 64), (1031, 776)])
def test_dropout_add(shape, p):
    from ringdp._native import C

    thr, scale = dc.quantize(p)
    x, res = _rand_bf16(shape, 2, 0.5), _rand_bf16(shape, 3, 0.5)
    seed, step, site = 1234, 2, 1
    y = C.dropout_add_bf16(x, res, _snap(seed, step), site, thr, 0, 0, 0)
    mask = _mask(shape, thr, seed, step, site)
    same = _bits(y) == _bits(res)
    # a kept element moves res by at least 0.5: the positions equal to res are exactly the dropped ones
    assert torch.equal(same, ~mask), int((same == mask).sum())
    v = res.double() + float(scale) * x.double()
    err = (y.double() - v).abs()
    assert bool((err[mask] <= _ulp_bf16(v)[mask]).all()), float((err / _ulp_bf16(v))[mask].max())


def test_row_mode():
    """B = 6 samples of T = 5 rows, p = 0.5, seed 1234, step 1, site 3: the oracle keeps samples {1, 5} only."""
    from ringdp._native import C

    B, T, N = 6, 5, 64
    thr, scale = dc.quantize(0.5)
    keep = dc.row_keep(B, thr, 1234, 1, 3)
    assert set(np.nonzero(keep)[0].tolist()) == {1, 5}
    x, res = _rand_bf16((B * T, N), 4, 0.5), _rand_bf16((B * T, N), 5, 0.5)
    snap = _snap(1234, 1)
    y = C.dropout_add_bf16(x, res, snap, 0, 0, 3, thr, T)
    rows = torch.from_numpy(np.repeat(keep, T)).to(DEV)
    assert torch.equal(_bits(y)[~rows], _bits(res)[~rows])
    v = res.double() + 2.0 * x.double()
    assert bool(((y.double() - v).abs()[rows] <= _ulp_bf16(v)[rows]).all())
    assert not bool((_bits(y)[rows] == _bits(res)[rows]).any())
    # the same factor without a residual (what the backward runs)
    z = C.dropout_bf16(x, snap, 0, 0, 3, thr, T)
    want = torch.where(rows[:, None], (x.float() * 2.0).bfloat16(), torch.zeros((), device=DEV, dtype=torch.bfloat16))
    assert torch.equal(_bits(z), _bits(want))
    # row mode and element mode together: m = m_row * m_elem
    thr_e, scale_e = dc.quantize(0.1)
    both = C.dropout_add_bf16(x, res, snap, 1, thr_e, 3, thr, T)
    m = _mask((B * T, N), thr_e, 1234, 1, 1) & rows[:, None]
    assert torch.equal(_bits(both) == _bits(res), ~m)
    v = res.double() + float(np.float32(2.0) * scale_e) * x.double()
    assert bool(((both.double() - v).abs()[m] <= _ulp_bf16(v)[m]).all())
    zb = C.dropout_bf16(x, snap, 1, thr_e, 3, thr, T)
    want = torch.where(m, (x.float() * float(np.float32(2.0) * scale_e)).bfloat16(),
                       torch.zeros((), device=DEV, dtype=torch.bfloat16))
    assert torch.equal(_bits(zb), _bits(want))


def test_backward():
    import ringdp.random as rr
    from ringdp.ops.dropout import DropoutAddF, DropoutF, dropout

    shape = (394, 64)
    thr, scale = dc.quantize(0.1)
    x = _rand_bf16(shape, 6).requires_grad_()
    dy = _rand_bf16(shape, 7)
    snap = _snap(77, 3)
    y = DropoutF.apply(x, snap, 2, thr)
    (dx,) = torch.autograd.grad(y, x, dy)
    mask = _mask(shape, thr, 77, 3, 2)
    assert torch.equal(_bits(dx), _bits(_want_dropout(dy, mask, scale)))
    # DropoutAddF: (m * dy, dy itself)
    res = _rand_bf16(shape, 8).requires_grad_()
    y = DropoutAddF.apply(x, res, snap, 2, thr, 0, 0, 0)
    dx, dres = torch.autograd.grad(y, (x, res), dy)
    assert torch.equal(_bits(dx), _bits(_want_dropout(dy, mask, scale)))
    assert torch.equal(_bits(dres), _bits(dy))

    class Ctx:  # the Function hands dy itself on: no copy, no pass over it
        needs_input_grad = (True, True)
        snapshot = snap
        cfg = (2, thr, 0, 0, 0)

    assert DropoutAddF.backward(Ctx, dy)[1] is dy
    # fwd(A), fwd(B), bwd(B), bwd(A): each backward regenerates its own forward's mask
    rr.manual_seed(99, DEV)
    xa, xb = _rand_bf16(shape, 9).requires_grad_(), _rand_bf16(shape, 10).requires_grad_()
    ya = dropout(xa, 0.1, True)
    yb = dropout(xb, 0.1, True)
    (dxb,) = torch.autograd.grad(yb, xb, dy)
    (dxa,) = torch.autograd.grad(ya, xa, dy)
    ma, mb = _mask(shape, thr, 99, 1, 0), _mask(shape, thr, 99, 2, 0)
    assert not torch.equal(ma, mb)
    assert torch.equal(_bits(ya), _bits(_want_dropout(xa.detach(), ma, scale)))
    assert torch.equal(_bits(yb), _bits(_want_dropout(xb.detach(), mb, scale)))
    assert torch.equal(_bits(dxa), _bits(_want_dropout(dy, ma, scale)))
    assert torch.equal(_bits(dxb), _bits(_want_dropout(dy, mb, scale)))


def test_state():
    import ringdp.nn as rnn
    import ringdp.random as rr
    from ringdp.ops.dropout import dropout

    x = torch.ones(394, 64, device=DEV, dtype=torch.bfloat16)
    seed = 2 ** 40 + 7
    rr.manual_seed(seed, DEV)
    assert rr.get_rng_state(DEV) == (seed, 0)
    first = [dropout(x, 0.5, True) for _ in range(3)]
    assert rr.get_rng_state(DEV) == (seed, 3)  # step counts the ticks
    thr, _ = dc.quantize(0.5)
    for k, y in enumerate(first):
        assert torch.equal(y != 0, _mask(x.shape, thr, seed, k + 1, 0))
    rr.manual_seed(seed, DEV)
    again = [dropout(x, 0.5, True) for _ in range(3)]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[0], first[1])
    # a state taken mid-sequence reproduces the next mask
    st = rr.get_rng_state(DEV)
    assert st == (seed, 3) and all(type(v) is int for v in st)
    nxt = dropout(x, 0.5, True)
    dropout(x, 0.5, True)
    rr.set_rng_state(st, DEV)
    assert torch.equal(dropout(x, 0.5, True), nxt)
    # the module: train draws, eval is the identity, sites of one draw differ
    m = rnn.Dropout(0.5)
    d = rr.Draw(DEV)
    a, b = m(x, d), m(x, d)
    assert not torch.equal(a, b)
    step = rr.get_rng_state(DEV)[1]
    assert torch.equal(a != 0, _mask(x.shape, thr, seed, step, 0))
    assert torch.equal(b != 0, _mask(x.shape, thr, seed, step, 1))
    assert m.eval()(x) is x


def test_graph_replay():
    """tick + dropout captured into one graph: every replay must draw the next step's mask.  A generator whose
    counter lived on the host would replay one mask for ever."""
    import ringdp.random as rr
    from ringdp.ops.dropout import dropout
    from ringdp.utils.graph import StepGraph

    x = torch.ones(394, 64, device=DEV, dtype=torch.bfloat16)
    rr.manual_seed(4321, DEV)

    def step_fn():
        return dropout(x, 0.5, True)

    graph = StepGraph(step_fn, warmup=3).capture()
    thr, _ = dc.quantize(0.5)
    got = []
    for _ in range(4):
        got.append(graph.replay().clone())
    torch.cuda.synchronize()
    for k, y in enumerate(got):
        assert torch.equal(y != 0, _mask(x.shape, thr, 4321, 4 + k, 0)), k
    assert all(not torch.equal(got[i], got[j]) for i in range(4) for j in range(i))
    assert rr.get_rng_state(DEV) == (4321, 7)


def test_errors_and_identity():
    import ringdp.random as rr
    from ringdp._native import C
    from ringdp.ops.dropout import dropout, dropout_add

    snap = _snap(1, 1)
    thr = dc.quantize(0.5)[0]
    x = torch.ones(8, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        C.dropout_bf16(x.float(), snap, 0, thr)
    with pytest.raises(TypeError):
        dropout(x.float(), 0.5, True)
    with pytest.raises(RuntimeError):
        C.dropout_bf16(torch.ones(8, 12, device=DEV, dtype=torch.bfloat16), snap, 0, thr)
    view = torch.ones(8 * 16 + 8, device=DEV, dtype=torch.bfloat16)[4:4 + 128].view(8, 16)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError):
        C.dropout_bf16(view, snap, 0, thr)
    with pytest.raises(RuntimeError):
        C.dropout_add_bf16(x, view, snap, 0, thr, 0, 0, 0)
    with pytest.raises(RuntimeError):
        C.dropout_bf16(x, snap.cpu(), 0, thr)
    with pytest.raises(RuntimeError):
        C.dropout_bf16(x[:, ::2], snap, 0, thr)
    with pytest.raises(RuntimeError):
        C.dropout_add_bf16(x, x, snap, 0, 0, 1, thr, 3)  # 8 rows are no whole samples of 3
    # p == 0: nothing is drawn or launched - the input itself / the existing add kernel
    rr.manual_seed(5, DEV)
    res = _rand_bf16((8, 16), 11)
    assert dropout(x, 0.0, True) is x
    assert dropout(x, 0.5, False) is x
    assert C.dropout_bf16(x, None, 0, 0).data_ptr() == x.data_ptr()
    y = dropout_add(x, res, 0.0, True)
    assert torch.equal(_bits(y), _bits(C.add_bf16(x, res)))
    assert rr.get_rng_state(DEV) == (5, 0)


# --------------------------------------------------------------------------------------------- model level
def _block_oracle(blk, x, masks, scale, emulate=True):
    """``test_model_parity_gpu._block_oracle`` with the three dropout masks injected where the GPU path applies
    them and bf16 rounding where it stores bf16: the out-proj output, each fused residual + dropout, the dropped
    GELU output."""
    import test_model_parity_gpu as P

    _rb = P._rbf if emulate else (lambda t: t)
    m0, m1, m2 = (m.to(x.dtype) * scale for m in masks)
    att = blk.self_attention
    B, T, D = x.shape
    H = att.num_heads
    dh = D // H
    h = _rb(F.layer_norm(x, (D,), blk.ln_1.weight, blk.ln_1.bias, blk.ln_1.eps))
    qkv = _rb(F.linear(h, _rb(att.in_proj_weight), att.in_proj_bias))
    q, k, v = qkv.split(D, -1)
    q, k, v = (t.reshape(B, T, H, dh).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), -1)
    o = _rb((_rb(p) @ v).transpose(1, 2).reshape(B, T, D))
    x = _rb(x + m0 * _rb(F.linear(o, _rb(att.out_proj.weight), att.out_proj.bias)))
    h = _rb(F.layer_norm(x, (D,), blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps))
    a = _rb(m1 * _rb(F.gelu(F.linear(h, _rb(blk.mlp[0].weight), blk.mlp[0].bias))))
    return _rb(x + m2 * _rb(F.linear(a, _rb(blk.mlp[3].weight), blk.mlp[3].bias)))


@pytest.mark.parametrize("heads,D,hidden,B,T", [(4, 64, 128, 6, 65), (12, 768, 3072, 2, 197)], ids=["small", "b16"])
def test_block_parity(heads, D, hidden, B, T):
    """One encoder block with dropout = 0.1 called on its own (it makes its own draw): ringdp and the
    bf16-storage oracle against the fp64 math, all three with the oracle masks of sites 0, 1, 2.  Gates as in
    ``test_vit_b16_block_vs_bf16_oracle``: parameter gradients through its ``_gate``; output at 1e-2 and input
    gradient at 2e-2, or twice the bf16 oracle's own error where that is larger."""
    import ringdp.random as rr
    import test_model_parity_gpu as P
    from ringdp.models.vit import EncoderBlock
    from ringdp.ops.transformer import cast_weights, clear_weights

    torch.manual_seed(0)
    blk = EncoderBlock(heads, D, hidden, dropout=0.1).cuda().train()
    orc = copy.deepcopy(blk)
    ref = copy.deepcopy(blk).double()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, T, D, device="cuda", generator=g).bfloat16()
    dy = torch.randn(B, T, D, device="cuda", generator=g).bfloat16()
    seed = 31337
    thr, scale = dc.quantize(0.1)
    masks = [_mask((B, T, n), thr, seed, 1, site) for site, n in ((0, D), (1, hidden), (2, D))]
    xo = x.float().requires_grad_()
    out_orc = _block_oracle(orc, xo, masks, float(scale))
    out_orc.backward(dy.float())
    xr = x.double().requires_grad_()
    out_ref = _block_oracle(ref, xr, masks, float(scale), emulate=False)
    out_ref.backward(dy.double())
    xm = x.reshape(B * T, D).clone().requires_grad_()
    att = blk.self_attention
    rr.manual_seed(seed, DEV)
    cast_weights([att.in_proj_weight, att.out_proj.weight, blk.mlp[0].weight, blk.mlp[3].weight])
    try:
        out = blk.forward_rows(xm, B, T)
    finally:
        clear_weights()
    assert rr.get_rng_state(DEV) == (seed, 1)
    assert out.shape == (B * T, D) and out.dtype == torch.bfloat16
    e_out = P._rel_l2(out.detach().view(B, T, D), out_ref.detach())
    o_out = P._rel_l2(out_orc.detach(), out_ref.detach())
    out.backward(dy.reshape(B * T, D))
    e_dx = P._rel_l2(xm.grad.view(B, T, D), xr.grad)
    o_dx = P._rel_l2(xo.grad, xr.grad)
    print(f"block D={D} B={B}: out {e_out:.2e} (oracle {o_out:.2e}) dx {e_dx:.2e} (oracle {o_dx:.2e})")
    named = list(zip(blk.named_parameters(), orc.parameters(), ref.parameters()))
    mine = {n: P._rel_l2(p.grad, r.grad) for (n, p), q, r in named}
    oracle = {n: P._rel_l2(q.grad, r.grad) for (n, p), q, r in named}
    assert e_out < max(1e-2, 2.0 * o_out), (e_out, o_out)
    assert e_dx < max(2e-2, 2.0 * o_dx), (e_dx, o_dx)
    P._gate(mine, oracle, f"vit block dropout D={D}")


def _tiny_pair(**kw):
    from ringdp.models import vit_tiny

    torch.manual_seed(0)
    base = vit_tiny().cuda()
    torch.nn.init.normal_(base.heads.head.weight, std=0.5)  # the zero-initialised head hides the encoder
    reg = vit_tiny(**kw).cuda()
    reg.load_state_dict(base.state_dict())
    return base, reg


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_vit_tiny_eval_is_unregularised(fp8):
    import ringdp.ops.transformer as tr
    from ringdp.ops.transformer import set_fp8

    base, reg = _tiny_pair(dropout=0.1, stochastic_depth_prob=0.1)
    x = torch.randn(16, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    tr._ROLLS.clear()
    set_fp8(fp8)
    try:
        with torch.no_grad():
            want = [base.eval()(x) for _ in range(2)]
            got = [reg.eval()(x) for _ in range(2)]
    finally:
        set_fp8(False)
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)


def test_vit_tiny_train():
    import ringdp.ops.transformer as tr
    import ringdp.random as rr
    from ringdp.ops.transformer import set_fp8

    _, reg = _tiny_pair(dropout=0.1, stochastic_depth_prob=0.1)
    reg.train()
    x = torch.randn(16, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    rr.manual_seed(11, DEV)
    with torch.no_grad():
        a, b = reg(x), reg(x)
    assert rr.get_rng_state(DEV) == (11, 2)  # one tick per forward
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    rr.manual_seed(11, DEV)
    with torch.no_grad():
        assert torch.equal(reg(x), a) and torch.equal(reg(x), b)
    # stochastic depth alone (no element dropout), and fp8 forward + backward
    _, sd = _tiny_pair(stochastic_depth_prob=0.5)
    sd.train()
    with torch.no_grad():
        outs = [sd(x) for _ in range(4)]
    assert all(torch.isfinite(o).all() for o in outs)
    assert any(not torch.equal(outs[0], o) for o in outs[1:])
    y = torch.randint(0, 10, (16,), device=DEV)
    tr._ROLLS.clear()
    set_fp8(True)
    try:
        for _ in range(2):  # the first call of each fp8 site measures its amax, the second takes the delayed path
            reg.zero_grad(set_to_none=True)
            loss = F.cross_entropy(reg(x), y)
            loss.backward()
    finally:
        set_fp8(False)
    assert math.isfinite(float(loss.detach()))
    grads = [p.grad for p in reg.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert sum(float(g.abs().sum()) for g in grads) > 0


def test_attention_dropout_raises():
    from ringdp.models.vit import EncoderBlock

    blk = EncoderBlock(4, 64, 128, attention_dropout=0.1).cuda().train()
    x = torch.zeros(2 * 65, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        blk.forward_rows(x, 2, 65)
    blk.eval().forward_rows(x, 2, 65)  # inference has no dropout: today's path


def test_captured_training_step():
    """forward + backward + AdamW of a regularised vit_tiny replayed from one hipGraph: the masks advance with the
    replays (the losses differ) and a restored generator state brings the same losses back bit for bit.  lr = 0
    keeps the weights, so the loss depends on the masks alone."""
    import ringdp
    import ringdp.random as rr
    from ringdp.nn import CrossEntropyLoss
    from ringdp.utils.graph import StepGraph

    _, model = _tiny_pair(dropout=0.1, stochastic_depth_prob=0.1)
    model.train()
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(16, 3, 32, 32, device=DEV, generator=g)
    y = torch.randint(0, 10, (16,), device=DEV, generator=g)
    opt = ringdp.optim.AdamW(model.parameters(), lr=torch.zeros((), device=DEV), weight_decay=1e-2)
    crit = CrossEntropyLoss()
    seed_grad = torch.ones((), device=DEV)

    def step_fn():
        loss = crit(model(x), y)
        opt.zero_grad(set_to_none=False)  # the gradient tensors (and the optimizer's pointer table) stay put
        loss.backward(seed_grad)
        opt.step()
        return loss

    rr.manual_seed(7, DEV)
    graph = StepGraph(step_fn, warmup=3).capture()
    state = rr.get_rng_state(DEV)
    assert state == (7, 3)
    first = [float(graph.replay()) for _ in range(4)]
    assert rr.get_rng_state(DEV) == (7, 7)
    assert all(math.isfinite(v) for v in first) and len(set(first)) > 1, first
    rr.set_rng_state(state, DEV)
    again = [float(graph.replay()) for _ in range(4)]
    assert again == first, (first, again)
