"""Key-blocked fused attention (T > 256: csrc/kernels/vit_attn_long.hip) against fp32 PyTorch softmax attention
with autograd on the same bf16 inputs, and the ViT at 325 tokens against its fp32 CPU reference.

Tolerances are the project's own for the fused attention kernels (forward rel < 1e-2, dqkv rel < 2e-2); a CPU
emulation of the blocked algorithm (P rounded to bf16 per block, D = rowsum(dO * O_bf16), dS rounded to bf16) sits
at 3e-3 .. 4.2e-3 on every shape used here."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = 0.125
KB = 128  # keys per staged block of the kernels (ATTL_KB)


def C():
    import ringdp

    return ringdp._C


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


def _tp(t):
    return (t + 15) // 16 * 16


def _inputs(B, T, H, spikes=False):
    g = torch.Generator(device=DEV).manual_seed(1000 * T + 10 * B + H)
    qkv = (torch.randn(B * T, 3 * H * 64, device=DEV, generator=g) * 0.5).bfloat16()
    dout = torch.randn(B * T, H * 64, device=DEV, generator=g).bfloat16()
    if spikes:
        v = qkv.view(B, T, 3, H, 64)
        v[:, 3, 0] = 2.0  # query 3 . key T - 2 = 256: scaled score 32, the maximum jumps in the last block
        v[:, T - 2, 1] = 2.0
        v[:, 40, 0] = -1.5  # query 40 . key KB + 5: the maximum jumps in a middle block and then stays
        v[:, KB + 5, 1] = -1.5
    return qkv, dout


def _reference(qkv, dout, B, T, H):
    """fp32 softmax attention with autograd: (out rows, lse [B*H, T], dqkv rows)."""
    leaf = qkv.float().requires_grad_()
    x = leaf.view(B, T, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * SCALE
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * T, H * 64)
    out.backward(dout.float())
    return out.detach(), torch.logsumexp(s.detach(), -1).reshape(B * H, T), leaf.grad


_CACHE = {}


def _case(B, T, H, spikes=False):
    """Inputs, the fp32 reference and one run of the kernels, computed once per shape and shared (read-only)."""
    key = (B, T, H, spikes)
    if key not in _CACHE:
        qkv, dout = _inputs(B, T, H, spikes)
        ref = _reference(qkv, dout, B, T, H)
        lse, out = C().attn_fwd_rows(qkv, B, T, H, SCALE, True)
        dqkv = C().attn_bwd_rows(dout, qkv, lse, B, T, H, SCALE, None, out)
        torch.cuda.synchronize()
        _CACHE[key] = (qkv, dout, ref, (out, lse, dqkv))
    return _CACHE[key]


@pytest.mark.parametrize("B,T,H", [(2, 257, 3), (1, 300, 3), (2, 512, 1), (2, 577, 3), (1, 1025, 1)])
def test_forward_backward_match_fp32(B, T, H):
    """257: a full key block plus a tile with one live key, last query tile with one live row; 300: a ragged
    block; 512: block-aligned, no masking; 577: ViT-B/16 at 384; 1025: nine key blocks, 17 query blocks."""
    _, _, (out_r, lse_r, dqkv_r), (out, lse, dqkv) = _case(B, T, H)
    Tp = _tp(T)
    assert out.shape == (B * T, H * 64) and out.dtype == torch.bfloat16
    assert dqkv.shape == (B * T, 3 * H * 64) and dqkv.dtype == torch.bfloat16
    assert lse.dtype == torch.float32 and lse.shape == (B * H, Tp)
    assert bool(torch.isposinf(lse[:, T:]).all())
    e_lse = float((lse[:, :T] - lse_r).abs().max())
    e_out, e_dqkv = rel(out, out_r), rel(dqkv, dqkv_r)
    print(f"T={T} B={B} H={H}: out {e_out:.2e} dqkv {e_dqkv:.2e} lse {e_lse:.2e}")
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    assert e_lse < 1e-3
    assert e_out < 1e-2
    assert e_dqkv < 2e-2


@pytest.mark.parametrize("T", [300, 577])
def test_forced_rescale(T):
    """Online-softmax rescale with the running maximum jumping by a lot in the last and in a middle key block:
    the spiked query rows and all other rows each against the fp32 reference over those same rows."""
    B, H = 2, 3
    _, _, (out_r, lse_r, dqkv_r), (out, lse, dqkv) = _case(B, T, H, spikes=True)
    for t in (out, dqkv, lse[:, :T]):
        assert bool(torch.isfinite(t.float()).all())
    spiked = torch.zeros(T, dtype=torch.bool, device=DEV)
    spiked[[3, 40]] = True
    for rows in (spiked, ~spiked):
        sel = rows.repeat(B)
        e_out, e_dqkv = rel(out[sel], out_r[sel]), rel(dqkv[sel], dqkv_r[sel])
        e_lse = float((lse.view(B * H, -1)[:, :T][:, rows] - lse_r[:, rows]).abs().max())
        print(f"T={T} rows={int(rows.sum())}: out {e_out:.2e} dqkv {e_dqkv:.2e} lse {e_lse:.2e}")
        assert e_out < 1e-2
        assert e_dqkv < 2e-2
        assert e_lse < 1e-3


@pytest.mark.parametrize("T", [197, 256])
def test_long_kernels_agree_with_short(T):
    B, H = 2, 3
    qkv, dout = _inputs(B, T, H)
    lse_s, out_s = C().attn_fwd_rows(qkv, B, T, H, SCALE, True)
    dqkv_s = C().attn_bwd_rows(dout, qkv, lse_s, B, T, H, SCALE)
    lse_l, out_l = C().attn_fwd_rows(qkv, B, T, H, SCALE, True, force_long=True)
    dqkv_l = C().attn_bwd_rows(dout, qkv, lse_l, B, T, H, SCALE, None, out_l, force_long=True)
    # without force_long the dispatch is the short kernels': bit-identical run to run
    lse_s2, out_s2 = C().attn_fwd_rows(qkv, B, T, H, SCALE, True)
    torch.cuda.synchronize()
    assert torch.equal(out_s, out_s2) and torch.equal(lse_s, lse_s2)
    assert lse_l.shape == lse_s.shape
    assert bool(torch.isposinf(lse_l[:, T:]).all())
    e_lse = float((lse_l[:, :T] - lse_s[:, :T]).abs().max())
    print(f"T={T}: out {rel(out_l, out_s):.2e} dqkv {rel(dqkv_l, dqkv_s):.2e} lse {e_lse:.2e}")
    assert rel(out_l, out_s) < 1e-2
    assert e_lse < 1e-3
    assert rel(dqkv_l, dqkv_s) < 1e-2


def test_bitwise_reproducible():
    B, T, H = 2, 577, 3
    qkv, dout, _, (out, lse, dqkv) = _case(B, T, H)
    lse2, out2 = C().attn_fwd_rows(qkv, B, T, H, SCALE, True)
    dqkv2 = C().attn_bwd_rows(dout, qkv, lse2, B, T, H, SCALE, None, out2)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)


@pytest.mark.parametrize("T", [300, 577])
def test_column_sum_partials(T):
    """The per-(batch, 64-row block) dq / dk / dv column sums of the key-blocked backward: every entry written,
    their sum the column sums of the dqkv rows stored (tolerances of
    test_attention_backward_column_sums_match_dqkv)."""
    B, H = 2, 3
    qkv, dout, _, (out, lse, dqkv) = _case(B, T, H)
    rows = C().attn_colsum_rows(B, T)
    assert rows == B * ((_tp(T) + 63) // 64)
    part = torch.full((rows, 3 * H * 64), float("nan"), device=DEV)
    got = C().attn_bwd_rows(dout, qkv, lse, B, T, H, SCALE, part, out)
    torch.cuda.synchronize()
    assert torch.equal(got, dqkv)
    assert bool(torch.isfinite(part).all())  # every entry written
    torch.testing.assert_close(part.sum(0), dqkv.float().sum(0), rtol=1e-4, atol=2e-3)
    red = torch.empty(3 * H * 64, device=DEV)
    C().rowsum_f32(part, red)
    torch.testing.assert_close(red, dqkv.float().sum(0), rtol=1e-4, atol=2e-3)


def _saved_shapes(fn):
    saved = []

    def pack(t):
        saved.append((tuple(t.shape), t.dtype))
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        fn()
    return saved


def test_dispatch(monkeypatch):
    import ringdp.ops.transformer as tr

    B, T, H = 2, 300, 3
    Tp = _tp(T)
    qkv, dout, (out_r, _, dqkv_r), _ = _case(B, T, H)
    res = {}

    def run():
        x = qkv.clone().requires_grad_()
        y = tr.AttentionF.apply(x, B, T, H)
        res["y"], res["x"] = y, x

    saved = _saved_shapes(run)
    assert ((B * H, Tp), torch.float32) in saved, saved  # the log-sum-exp
    assert not any(len(s) == 3 and s[-2:] == (Tp, Tp) for s, _ in saved), saved  # no P
    res["y"].backward(dout)
    assert rel(res["y"].detach(), out_r) < 1e-2 and rel(res["x"].grad, dqkv_r) < 2e-2
    # the GEMM path is still reachable, at every length
    monkeypatch.setattr(tr, "_ATTN_UNFUSED", True)
    saved = _saved_shapes(run)
    assert ((B * H, Tp, Tp), torch.bfloat16) in saved, saved
    assert rel(res["y"].detach(), out_r) < 1e-2
    with pytest.raises(RuntimeError, match="256"):
        C().attn_fwd_rows(qkv, B, T, H, SCALE, False)
    with pytest.raises(RuntimeError, match="out"):
        C().attn_bwd_rows(dout, qkv, _case(B, T, H)[3][1], B, T, H, SCALE)


def test_qkv_bias_gradient_through_linear():
    """LinearF takes the attention backward's partials for the qkv projection's bias gradient at T > 256 too."""
    import ringdp.ops.transformer as tr

    B, T, H = 2, 300, 2
    D = H * 64
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (torch.randn(B * T, D, device=DEV, generator=g)).bfloat16()
    lin = torch.nn.Linear(D, 3 * D).to(DEV)
    dout = torch.randn(B * T, D, device=DEV, generator=g).bfloat16()
    grads = {}
    qkv = tr.linear(x, lin)
    qkv.register_hook(lambda gr: grads.__setitem__("dqkv", gr.detach().clone()))
    tr.AttentionF.apply(qkv, B, T, H).backward(dout)
    torch.cuda.synchronize()
    torch.testing.assert_close(lin.bias.grad.float(), grads["dqkv"].float().sum(0), rtol=1e-4, atol=2e-3)


def _cos(a, b):
    return float(F.cosine_similarity(a.reshape(1, -1).float().cpu(), b.reshape(1, -1).float().cpu()))


def _vit325():
    from ringdp.models import VisionTransformer

    torch.manual_seed(0)
    m = VisionTransformer(image_size=72, patch_size=4, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256,
                          num_classes=10)
    torch.nn.init.normal_(m.heads.head.weight, std=0.05)  # zero-initialised: logits would all be 0
    return m


def test_vit_325_tokens_matches_cpu_reference():
    m = _vit325()
    assert m.seq_length == 325
    ref = copy.deepcopy(m)
    m = m.to(DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 72, 72, generator=g)
    y = torch.randint(0, 10, (2,), generator=g)
    out = m(x.to(DEV))
    out_ref = ref.reference_forward(x)
    assert out.shape == (2, 10) and out.dtype == torch.float32
    c_out = _cos(out.detach(), out_ref.detach())
    F.cross_entropy(out, y.to(DEV)).backward()
    F.cross_entropy(out_ref, y).backward()
    cos = {n: _cos(p.grad, q.grad) for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters())}
    print(f"logits cos {c_out:.5f}; min grad cos {min(cos.values()):.5f} ({min(cos, key=cos.get)})")
    assert c_out > 0.99
    bad = {n: round(c, 4) for n, c in cos.items() if not c > 0.95}
    assert not bad, bad


def test_vit_325_tokens_captured_step():
    """forward + backward + SGD.step at 325 tokens captured once and replayed twice: the first replay's loss is
    the eager step's, bit for bit.  Two warm-up steps come first on both sides (SGD builds its pointer table
    with a host copy on the first step; the gradient tensors stay put), so the replays are steps 3 and 4."""
    from ringdp.optim import SGD
    from ringdp.utils.graph import StepGraph

    m0 = _vit325().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(2, 3, 72, 72, device=DEV, generator=g)
    y = torch.randint(0, 10, (2,), device=DEV, generator=g)

    def make():
        m = copy.deepcopy(m0)
        opt = SGD(m.parameters(), lr=0.05, momentum=0.9)

        def step():
            loss = F.cross_entropy(m(x), y)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            opt.step()
            return loss

        return step

    eager = make()
    l_eager = [eager().detach().clone() for _ in range(4)]
    graph = StepGraph(make(), warmup=2).capture()  # the capture itself executes nothing
    l_graph = [graph.replay().clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(l_graph[0], l_eager[2]), (l_graph, l_eager)
    assert math.isfinite(float(l_graph[1])) and float(l_graph[1]) != float(l_graph[0])
