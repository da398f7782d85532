"""Attention dropout inside the fused attention kernels (csrc/kernels/vit_attn_drop.hip) against fp64 PyTorch
attention with the mask of the numpy Philox oracle, written from the definition in ``ringdp.ops.dropout``
(attention mode).  Error measure and bounds are those of ``test_attention_long_gpu`` (the same arithmetic)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_common as dc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SCALE = 0.125
SEED, STEP, SITE = 2 ** 63 + 2 ** 40 + 7, 2 ** 32 + 5, 3


def C():
    import ringdp

    return ringdp._C


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _snap(seed, step):
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed, step)], dtype=torch.int64, device=DEV)


def _quantize8(p):
    thr8 = min(max(int(round(p * 256.0)), 0), 255)
    return thr8, float(np.float32(256.0 / (256 - thr8)))


def keep_mask(B, H, T, thr8, seed, step, site):
    """The [B, H, T, T] keep array: one Philox call per 4 x 4 tile of (query, key), 8-bit draws."""
    n4 = (T + 3) // 4
    bh, tq, tk = np.ogrid[:B * H, :T, :T]
    tiles = (np.arange(B * H * n4 * n4, dtype=np.uint64)).reshape(B * H, n4, n4)  # ((b*H + h)*N4 + tq/4)*N4 + tk/4
    w = np.stack(dc.philox4x32_10(tiles, step & 0xFFFFFFFF, step >> 32, site, seed & 0xFFFFFFFF, seed >> 32))
    u8 = (w[tq & 3, bh, tq >> 2, tk >> 2] >> (8 * (tk & 3)).astype(np.uint32)) & np.uint32(0xFF)
    return torch.from_numpy((u8 >= thr8).reshape(B, H, T, T)).to(DEV)


def _reference(qkv, dout, keep, scale_keep, B, T, H):
    """fp64 attention with the mask on the probabilities: (out rows, lse of the undropped softmax, dqkv, Pd)."""
    leaf = qkv.double().requires_grad_()
    x = leaf.view(B, T, 3, H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * SCALE
    pd = torch.softmax(s, -1) * keep.double() * scale_keep
    out = (pd @ v).permute(0, 2, 1, 3).reshape(B * T, H * 64)
    out.backward(dout.double())
    return out.detach(), torch.logsumexp(s.detach(), -1).reshape(B * H, T), leaf.grad, pd.detach()


def _inputs(B, T, H):
    g = torch.Generator(device=DEV).manual_seed(1000 * T + 10 * B + H)
    qkv = (torch.randn(B * T, 3 * H * 64, device=DEV, generator=g) * 0.5).bfloat16()
    return qkv, torch.randn(B * T, H * 64, device=DEV, generator=g).bfloat16()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_exact_mask(p):
    """V[k] = one-hot(k), so out[q, k] = Pd[q, k]: the zero pattern is the oracle's keep array exactly (a transposed
    tile, a wrong word or byte, a wrong bh / N4 in the counter all show), at a T that is no multiple of 4."""
    B, H, T = 2, 2, 61
    thr8, scale_keep = _quantize8(p)
    qkv, dout = _inputs(B, T, H)
    qkv.view(B, T, 3, H, 64)[:, :, 2] = torch.eye(T, 64, device=DEV, dtype=torch.bfloat16)[None, :, None, :]
    keep = keep_mask(B, H, T, thr8, SEED, STEP, SITE)
    _, out = C().attn_drop_fwd_rows(qkv, B, T, H, SCALE, _snap(SEED, STEP), SITE, thr8)
    got = out.view(B, T, H, 64).permute(0, 2, 1, 3)[..., :T]
    assert 0.8 * (1 - p) < float(keep.float().mean()) < min(1.0, 1.2 * (1 - p))
    assert torch.equal(got != 0, keep), int(((got != 0) != keep).sum())
    assert not bool((out.view(B, T, H, 64)[..., T:] != 0).any())
    pd = _reference(qkv, dout, keep, scale_keep, B, T, H)[3]
    assert rel(got, pd) < 1e-2


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,T,H", [(2, 5, 1), (2, 65, 2), (1, 197, 3), (2, 261, 2)])
def test_forward_backward_match_fp64(B, T, H, p):
    """5: one partial tile; 65: a workgroup edge; 197: the ViT length; 261: two 128-key blocks and a ragged tail."""
    thr8, scale_keep = _quantize8(p)
    qkv, dout = _inputs(B, T, H)
    snap = _snap(SEED, STEP)
    out_r, lse_r, dqkv_r, _ = _reference(qkv, dout, keep_mask(B, H, T, thr8, SEED, STEP, SITE), scale_keep, B, T, H)
    lse, out = C().attn_drop_fwd_rows(qkv, B, T, H, SCALE, snap, SITE, thr8)
    part = torch.full((C().attn_colsum_rows(B, T, True), 3 * H * 64), float("nan"), device=DEV)
    dqkv = C().attn_drop_bwd_rows(dout, qkv, lse, out, B, T, H, SCALE, snap, SITE, thr8, part)
    Tp = (T + 15) // 16 * 16
    assert out.shape == (B * T, H * 64) and dqkv.shape == qkv.shape and lse.shape == (B * H, Tp)
    assert bool(torch.isposinf(lse[:, T:]).all())
    e_lse = float((lse[:, :T].double() - lse_r).abs().max())
    e_out, e_dqkv = rel(out, out_r), rel(dqkv, dqkv_r)
    print(f"T={T} B={B} H={H} p={p}: out {e_out:.2e} dqkv {e_dqkv:.2e} lse {e_lse:.2e}")
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    assert e_lse < 1e-3
    assert e_out < 1e-2
    assert e_dqkv < 2e-2
    assert bool(torch.isfinite(part).all())  # every entry written
    torch.testing.assert_close(part.sum(0), dqkv.float().sum(0), rtol=1e-4, atol=2e-3)


def test_state():
    B, T, H = 2, 65, 2
    thr8 = _quantize8(0.1)[0]
    qkv, dout = _inputs(B, T, H)

    def run(step, site):
        snap = _snap(SEED, step)
        lse, out = C().attn_drop_fwd_rows(qkv, B, T, H, SCALE, snap, site, thr8)
        return out, C().attn_drop_bwd_rows(dout, qkv, lse, out, B, T, H, SCALE, snap, site, thr8)

    (o1, d1), (o2, d2) = run(STEP, SITE), run(STEP, SITE)
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    assert not torch.equal(run(STEP + 1, SITE)[0], o1) and not torch.equal(run(STEP, SITE + 1)[0], o1)
    snap = _snap(SEED, STEP)
    for heads, sn, t8 in ((H, snap, 0), (H, snap, 256), (H, None, thr8), (8, snap, thr8)):  # 8 heads: head dim 16
        with pytest.raises(RuntimeError):
            C().attn_drop_fwd_rows(qkv, B, T, heads, SCALE, sn, SITE, t8)


def _block_ref(blk, x, keep, scale_keep):
    """fp64 math of one encoder block with the attention mask on the probabilities."""
    att, (B, T, D), H = blk.self_attention, x.shape, blk.self_attention.num_heads
    qkv = F.linear(F.layer_norm(x, (D,), blk.ln_1.weight, blk.ln_1.bias, blk.ln_1.eps), att.in_proj_weight,
                   att.in_proj_bias)
    q, k, v = (t.reshape(B, T, H, D // H).transpose(1, 2) for t in qkv.split(D, -1))
    pd = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // H), -1) * keep.double() * scale_keep
    x = x + att.out_proj((pd @ v).transpose(1, 2).reshape(B, T, D))
    return x + blk.mlp(F.layer_norm(x, (D,), blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps))


def test_block():
    import ringdp.random as rr
    from ringdp.models.vit import EncoderBlock
    from ringdp.ops.transformer import cast_weights, clear_weights

    B, T, H, D = 2, 65, 2, 128
    torch.manual_seed(0)
    blk = EncoderBlock(H, D, 256, attention_dropout=0.25).cuda().train()
    plain = EncoderBlock(H, D, 256).cuda().eval()
    plain.load_state_dict(blk.state_dict())
    ref = copy.deepcopy(blk).double()
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, T, D, device="cuda", generator=g).bfloat16()
    dy = torch.randn(B, T, D, device="cuda", generator=g).bfloat16()
    thr8, scale_keep = _quantize8(0.25)
    xr = x.double().requires_grad_()
    out_ref = _block_ref(ref, xr, keep_mask(B, H, T, thr8, 31337, 1, 0), scale_keep)  # the block's first site
    out_ref.backward(dy.double())

    def rows(b, inp):
        att = b.self_attention
        cast_weights([att.in_proj_weight, att.out_proj.weight, b.mlp[0].weight, b.mlp[3].weight])
        try:
            return b.forward_rows(inp, B, T)
        finally:
            clear_weights()

    rr.manual_seed(31337, DEV)
    xm = x.reshape(B * T, D).clone().requires_grad_()
    out = rows(blk, xm)
    assert rr.get_rng_state(DEV) == (31337, 1)
    out.backward(dy.reshape(B * T, D))
    e_out, e_dx = rel(out.detach().view(B, T, D), out_ref.detach()), rel(xm.grad.view(B, T, D), xr.grad)
    print(f"block: out {e_out:.2e} dx {e_dx:.2e}")
    assert e_out < 1e-2
    assert e_dx < 2e-2
    with torch.no_grad():
        assert torch.equal(rows(blk.eval(), x.reshape(B * T, D)), rows(plain, x.reshape(B * T, D)))
    assert rr.get_rng_state(DEV) == (31337, 1)  # eval draws nothing


def test_captured_training_step():
    """test_dropout_gpu.test_captured_training_step with attention dropout alone, 12 heads x 64 at 5 tokens."""
    import ringdp
    import ringdp.random as rr
    from ringdp.models import VisionTransformer
    from ringdp.nn import CrossEntropyLoss
    from ringdp.utils.graph import StepGraph

    torch.manual_seed(0)
    model = VisionTransformer(image_size=32, patch_size=16, num_layers=1, num_heads=12, hidden_dim=768, mlp_dim=768,
                              num_classes=10, attention_dropout=0.1).cuda().train()
    torch.nn.init.normal_(model.heads.head.weight, std=0.5)  # the zero-initialised head hides the encoder
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(8, 3, 32, 32, device=DEV, generator=g)
    y = torch.randint(0, 10, (8,), device=DEV, generator=g)
    opt = ringdp.optim.AdamW(model.parameters(), lr=torch.zeros((), device=DEV), weight_decay=1e-2)
    crit = CrossEntropyLoss()
    seed_grad = torch.ones((), device=DEV)

    def step_fn():
        loss = crit(model(x), y)
        opt.zero_grad(set_to_none=False)
        loss.backward(seed_grad)
        opt.step()
        return loss

    rr.manual_seed(7, DEV)
    graph = StepGraph(step_fn, warmup=3).capture()
    state = rr.get_rng_state(DEV)
    assert state == (7, 3)
    first = [float(graph.replay()) for _ in range(3)]
    assert all(math.isfinite(v) for v in first) and len(set(first)) == 3, first
    rr.set_rng_state(state, DEV)
    assert [float(graph.replay()) for _ in range(3)] == first
