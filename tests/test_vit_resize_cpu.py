"""Position-embedding resize for fine-tuning a ViT at another resolution, and the constructor's
attention_dropout (CPU)."""
import pytest
import torch
import torch.nn.functional as F

from ringdp.models import VisionTransformer
from ringdp.models.vit import interpolate_pos_embedding


def _pos(n, d, seed=0):
    return torch.randn(1, 1 + n * n, d, generator=torch.Generator().manual_seed(seed))


def test_identity_at_equal_length():
    pos = _pos(14, 8)
    assert interpolate_pos_embedding(pos, 197) is pos


def test_resize_matches_direct_interpolate():
    pos = _pos(14, 8)
    out = interpolate_pos_embedding(pos, 1 + 24 * 24)
    assert out.shape == (1, 1 + 24 * 24, 8) and out.dtype == pos.dtype
    assert torch.equal(out[:, 0], pos[:, 0])  # class row copied
    grid = pos[0, 1:].t().reshape(1, 8, 14, 14)
    want = F.interpolate(grid, size=(24, 24), mode="bicubic", align_corners=True)
    assert torch.equal(out[0, 1:], want.reshape(8, 24 * 24).t())
    # align_corners: the grid's corners are kept
    assert torch.allclose(out[0, 1], pos[0, 1], atol=1e-6) and torch.allclose(out[0, -1], pos[0, -1], atol=1e-6)


def test_other_modes_and_dtypes():
    pos = _pos(4, 8).bfloat16()
    out = interpolate_pos_embedding(pos, 1 + 6 * 6, interpolation="bilinear")
    assert out.dtype == torch.bfloat16 and out.shape == (1, 37, 8)
    grid = pos[0, 1:].float().t().reshape(1, 8, 4, 4)
    want = F.interpolate(grid, size=(6, 6), mode="bilinear", align_corners=True).reshape(8, 36).t().bfloat16()
    assert torch.equal(out[0, 1:], want)
    assert interpolate_pos_embedding(_pos(4, 8), 1 + 2 * 2).shape == (1, 5, 8)  # downsizing


def test_rejects_non_square_lengths():
    with pytest.raises(ValueError):
        interpolate_pos_embedding(_pos(14, 8), 200)
    with pytest.raises(ValueError):
        interpolate_pos_embedding(torch.zeros(1, 200, 8), 197)
    with pytest.raises(ValueError):
        interpolate_pos_embedding(torch.zeros(197, 8), 197)


def test_constant_grid_stays_constant():
    pos = torch.full((1, 1 + 14 * 14, 8), 0.75)
    pos[:, 0] = -2.0
    out = interpolate_pos_embedding(pos, 1 + 24 * 24)
    assert torch.allclose(out[:, 1:], torch.full_like(out[:, 1:], 0.75), atol=1e-6)
    assert torch.equal(out[:, 0], pos[:, 0])


def _small(image_size, **kw):
    return VisionTransformer(image_size=image_size, patch_size=4, num_layers=2, num_heads=2, hidden_dim=32,
                             mlp_dim=64, num_classes=5, **kw)


def test_load_state_dict_resizes_position_embedding():
    torch.manual_seed(0)
    src, dst = _small(32), _small(48)
    sd = src.state_dict()
    with pytest.raises(RuntimeError, match="pos_embedding"):
        dst.load_state_dict(sd)
    keys = dst.load_state_dict(sd, resize_pos_embedding=True)
    assert not keys.missing_keys and not keys.unexpected_keys
    assert sd["encoder.pos_embedding"].shape == (1, 65, 32)  # the caller's dict is untouched
    got = dst.state_dict()
    for name, t in sd.items():
        if name == "encoder.pos_embedding":
            assert got[name].shape == (1, 145, 32)
            assert torch.equal(got[name], interpolate_pos_embedding(t, 145))
        else:
            assert torch.equal(got[name], t), name
    # equal shapes: the flag changes nothing
    same = _small(32)
    same.load_state_dict(sd, resize_pos_embedding=True)
    assert torch.equal(same.encoder.pos_embedding, src.encoder.pos_embedding)
    out = dst(torch.randn(2, 3, 48, 48))
    assert out.shape == (2, 5) and bool(torch.isfinite(out).all())


def test_attention_dropout_reaches_every_block():
    m = _small(32, attention_dropout=0.1)
    assert all(blk.self_attention.dropout == 0.1 for blk in m.encoder.layers)
    assert all(blk.self_attention.dropout == 0.0 for blk in _small(32).encoder.layers)
