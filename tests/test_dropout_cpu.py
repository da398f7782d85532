"""Dropout / stochastic depth: what can be checked without a GPU - the Philox oracle against the published
known answers, the probability quantisation, the default seed, the drop-path schedule, the statistics of the oracle
masks, and the ATen model path with ``stochastic_depth_prob``."""
import itertools
import math

import numpy as np
import pytest
import torch

import dropout_common as dc
from ringdp.ops.dropout import drop_path_schedule, quantize_p
from ringdp.random import default_seed


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w[0]) for w in dc.philox4x32_10(*ctr, *key))
    assert got == want, [hex(g) for g in got]


def test_quantize_p():
    assert quantize_p(0.0)[0] == 0
    assert quantize_p(0.1)[0] == 6554
    assert quantize_p(0.5) == (32768, 2.0)
    assert quantize_p(1 - 2 ** -17)[0] == 65535
    for p in (0.0, 0.1, 0.5, 1 - 2 ** -17):
        thr, scale = quantize_p(p)
        assert (thr, scale) == (dc.quantize(p)[0], float(dc.quantize(p)[1]))
        # scale is an fp32 value: the inverse of the realised keep probability (65536 - thr) / 65536 in fp32
        assert np.float32(scale) == scale
        assert np.float32(scale) * np.float32(65536 - thr) == np.float32(65536.0), (p, thr, scale)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            quantize_p(bad)


def test_default_seed():
    assert default_seed(1234, 0) == 1234
    assert default_seed(1234, 3) == 1237
    assert len({default_seed(7, r) for r in range(8)}) == 8  # no two ranks share masks
    assert default_seed(2 ** 64 - 1, 2) == 1  # wraps into the u64 the kernels read


def test_drop_path_schedule():
    assert drop_path_schedule(0.1, 1) == [0.0]
    assert drop_path_schedule(0.0, 4) == [0.0] * 4
    got = drop_path_schedule(0.1, 12)
    assert got[0] == 0.0 and got[-1] == pytest.approx(0.1)
    assert got == pytest.approx([0.1 * l / 11 for l in range(12)])
    from ringdp.models import vit_tiny

    m = vit_tiny(stochastic_depth_prob=0.2)
    assert [blk.drop_path for blk in m.encoder.layers] == pytest.approx([0.0, 0.2])
    assert [blk.drop_path for blk in vit_tiny().encoder.layers] == [0.0, 0.0]


@pytest.mark.parametrize("numel", [394 * 64, 394 * 128, 1000 * 768])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_oracle_kept_count(numel, p):
    """The kept count of every (seed, step, site) is within 5 sigma of numel * q (binomial)."""
    thr, _ = dc.quantize(p)
    q = (65536 - thr) / 65536
    sigma = math.sqrt(numel * q * (1 - q))
    worst = 0.0
    for seed, step, site in itertools.product((0, 1234, 2 ** 40 + 7), (1, 2, 3), (0, 1, 5)):
        kept = int(dc.element_keep(numel, thr, seed, step, site).sum())
        worst = max(worst, abs(kept - numel * q) / sigma)
        assert abs(kept - numel * q) <= 5 * sigma, (seed, step, site, kept, numel * q, sigma)
    print(f"numel {numel} p {p}: worst deviation {worst:.2f} sigma")


def test_oracle_masks_independent():
    """Masks of two steps, or of two sites, agree on 50 % +- 2 % of the positions at p = 0.5."""
    numel, thr = 1000 * 768, dc.quantize(0.5)[0]
    a = dc.element_keep(numel, thr, 1234, 1, 0)
    steps = float((a == dc.element_keep(numel, thr, 1234, 2, 0)).mean())
    sites = float((a == dc.element_keep(numel, thr, 1234, 1, 1)).mean())
    seeds = float((a == dc.element_keep(numel, thr, 1235, 1, 0)).mean())
    print(f"agreement: steps {steps:.4f} sites {sites:.4f} seeds {seeds:.4f}")
    for v in (steps, sites, seeds):
        assert abs(v - 0.5) <= 0.02, v


def test_oracle_row_mode_samples():
    """The row-mode case the GPU test uses: B = 6, p = 0.5, seed 1234, step 1, site 3 keeps samples {1, 5}."""
    keep = dc.row_keep(6, dc.quantize(0.5)[0], 1234, 1, 3)
    assert set(np.nonzero(keep)[0].tolist()) == {1, 5}, keep


def test_cpu_model_stochastic_depth():
    from ringdp.models import vit_tiny

    torch.manual_seed(0)
    base = vit_tiny()
    # a zero head (the init) hides everything upstream: give it weights
    torch.nn.init.normal_(base.heads.head.weight, std=0.1)
    reg = vit_tiny(dropout=0.1, stochastic_depth_prob=0.5)
    reg.load_state_dict(base.state_dict())  # same names: dropout adds no parameters or buffers
    x = torch.randn(4, 3, 32, 32)
    base.eval()
    reg.eval()
    assert torch.equal(reg(x), base(x))
    reg.train()
    torch.manual_seed(1)
    y1 = reg(x)
    y2 = reg(x)
    assert not torch.equal(y1, y2)
    torch.manual_seed(1)
    assert torch.equal(reg(x), y1)
    assert torch.isfinite(y1).all()
    y1.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in reg.parameters() if p.grad is not None)


def test_block_path_predicate_follows_the_thresholds():
    """The GPU block takes the dropout path exactly when a quantised threshold is non-zero (or attention dropout
    has to raise), in training mode only."""
    from ringdp.models.vit import EncoderBlock

    assert not EncoderBlock(4, 64, 128).train()._regularised()
    assert EncoderBlock(4, 64, 128, dropout=0.1).train()._regularised()
    assert not EncoderBlock(4, 64, 128, dropout=0.1).eval()._regularised()
    assert EncoderBlock(4, 64, 128, drop_path=0.1).train()._regularised()
    assert EncoderBlock(4, 64, 128, attention_dropout=0.1).train()._regularised()
    tiny = 2.0 ** -19  # rounds to threshold 0: nothing would be dropped, so the fused path stays
    assert quantize_p(tiny)[0] == 0
    assert not EncoderBlock(4, 64, 128, dropout=tiny, drop_path=tiny).train()._regularised()


def test_cpu_dropout_goes_to_aten():
    import ringdp.nn as rnn
    from ringdp.ops.dropout import dropout

    x = torch.ones(64, 64)
    assert dropout(x, 0.5, training=False) is x
    assert dropout(x, 0.0, training=True) is x
    torch.manual_seed(3)
    y = dropout(x, 0.5, training=True)
    torch.manual_seed(3)
    assert torch.equal(y, torch.nn.functional.dropout(x, 0.5, True))
    m = rnn.Dropout(0.5)
    assert set(m(x).unique().tolist()) == {0.0, 2.0}
    assert m.eval()(x) is x
    assert not list(m.state_dict())
