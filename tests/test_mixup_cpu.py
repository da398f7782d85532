"""Mixup / CutMix without a GPU: ``MixedTarget``, argument validation, the CPU path of ``ringdp.data.Mixup``
(pairing, box rule, labels), the record invariants on host-drawn records, and ``CrossEntropyLoss`` with a
``MixedTarget`` against the formula written out by hand."""
import math

import numpy as np
import pytest
import torch

import mixup_common as mc


def test_mixed_target_dense():
    from ringdp.ops.mixup import MixedTarget

    y_a, y_b = torch.tensor([0, 2, 1]), torch.tensor([1, 2, 0])
    t = MixedTarget(y_a, y_b, torch.tensor([0.25]))
    want = torch.tensor([[0.25, 0.75, 0.0], [0.0, 0.0, 1.0], [0.75, 0.25, 0.0]])
    assert torch.equal(t.dense(3), want)
    s = t.dense(3, label_smoothing=0.3)
    assert torch.allclose(s, 0.7 * want + 0.1) and torch.allclose(s.sum(1), torch.ones(3))
    # per-sample lam, also as a strided view (word 0 of a record tensor)
    rec = torch.zeros(3, 8)
    rec[:, 0] = torch.tensor([1.0, 0.5, 0.0])
    lam = rec[:, 0]
    assert lam.stride(0) == 8
    d = MixedTarget(y_a, y_b, lam).dense(3)
    assert torch.equal(d, torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]))
    for bad in (torch.tensor([0.5, 0.5]), torch.tensor([0.5], dtype=torch.float64), torch.tensor(0.5)):
        with pytest.raises(ValueError):
            MixedTarget(y_a, y_b, bad)
    with pytest.raises(ValueError):
        MixedTarget(y_a, y_b[:2], torch.tensor([0.5]))


def test_arguments():
    from ringdp.data import Mixup

    for kw in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(prob=1.5), dict(prob=-0.1),
               dict(switch_prob=2.0), dict(mode="pair"), dict(mode="half")):
        with pytest.raises(ValueError):
            Mixup(**kw)
    m = Mixup(0.8, 1.0)
    with pytest.raises(ValueError):
        m(torch.zeros(4, 3, 8), torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError):
        m(torch.zeros(4, 3, 8, 8), torch.zeros(3, dtype=torch.long))
    # eval, or both alphas 0: the input itself and lam = 1
    x, y = torch.randn(4, 3, 8, 8), torch.arange(4)
    for mod in (Mixup(0.8, 1.0).eval(), Mixup(0.0, 0.0)):
        out, t = mod(x, y)
        assert out is x and torch.equal(t.y_a, y) and torch.equal(t.lam, torch.ones(1))
        assert torch.equal(t.dense(4), torch.eye(4))


@pytest.mark.parametrize("H,W", [(7, 9), (32, 32), (224, 224)])
def test_host_records_satisfy_the_invariants(H, W):
    from ringdp.data.mixup import cpu_records

    torch.manual_seed(H)
    f = mc.check_records(cpu_records(256, H, W, 0.8, 1.0, 0.8, 0.5).numpy(), H, W)
    assert set(f["kind"].tolist()) == {0, 1, 2}
    assert np.all(mc.check_records(cpu_records(64, H, W, 0.8, 1.0, 0.0, 0.5).numpy(), H, W)["kind"] == 0)
    assert np.all(mc.check_records(cpu_records(64, H, W, 0.8, 1.0, 1.0, 0.0).numpy(), H, W)["kind"] == 1)
    assert np.all(mc.check_records(cpu_records(64, H, W, 0.8, 1.0, 1.0, 1.0).numpy(), H, W)["kind"] == 2)
    assert np.all(mc.check_records(cpu_records(64, H, W, 0.0, 1.0, 1.0, 0.5).numpy(), H, W)["kind"] == 2)
    assert np.all(mc.check_records(cpu_records(64, H, W, 0.8, 0.0, 1.0, 0.5).numpy(), H, W)["kind"] == 1)


def test_check_records_rejects_bad_records():
    """The invariant checker is the GPU tests' yardstick: it has to notice a wrong record."""
    good = np.stack([mc.make_record(float(mc.box_lam(2, 6, 1, 4, 8, 8)), 2, (2, 6, 1, 4), lam0=0.6)])
    mc.check_records(good, 8, 8)
    for bad in (mc.make_record(0.5, 0), mc.make_record(0.5, 1, (0, 1, 0, 1)), mc.make_record(0.5, 2, (2, 6, 1, 4), 0.6),
                mc.make_record(float(mc.box_lam(2, 9, 1, 4, 8, 8)), 2, (2, 9, 1, 4), 0.1),
                mc.make_record(float(mc.box_lam(0, 8, 0, 8, 8, 8)), 2, (0, 8, 0, 8), 0.9)):
        with pytest.raises(AssertionError):
            mc.check_records(np.stack([bad]), 8, 8)
    assert mc.ks_distance([0.0, 1.0], [0.0, 1.0]) == 0.0 and mc.ks_distance([0.0, 0.1], [0.9, 1.0]) == 1.0


@pytest.mark.parametrize("mode", ["batch", "elem"])
@pytest.mark.parametrize("B", [4, 5])
def test_cpu_path(mode, B):
    """Pairing with the flipped batch, the box rule and the labels, checked through values that name their sample:
    x[b] is the constant b + 1."""
    from ringdp.data import Mixup

    H, W = 8, 10
    x = (torch.arange(B, dtype=torch.float32) + 1).view(B, 1, 1, 1).expand(B, 3, H, W).contiguous()
    y = torch.arange(B) * 2
    torch.manual_seed(3)
    seen = set()
    for mix in (Mixup(0.8, 0.0, mode=mode), Mixup(0.0, 1.0, mode=mode), Mixup(0.8, 1.0, prob=0.6, mode=mode)):
        for _ in range(6):
            out, t = mix(x, y)
            assert out.shape == x.shape and out.dtype == x.dtype
            assert torch.equal(t.y_a, y) and torch.equal(t.y_b, y.flip(0))
            lam = t.lam.expand(B) if t.lam.numel() == 1 else t.lam
            assert lam.shape == (B,) and bool(((lam >= 0) & (lam <= 1)).all())
            for b in range(B):
                own, other = float(b + 1), float(B - b)
                img = out[b]
                assert torch.equal(img[0], img[1]) and torch.equal(img[0], img[2])  # every channel alike
                vals = set(img.unique().tolist())
                if own == other:
                    assert vals == {own}
                elif vals <= {own, other}:  # not applied, or a cutmix box: the share of own pixels is lam
                    share = float((img[0] == own).float().mean())
                    assert abs(share - float(lam[b])) < 1e-6, (share, float(lam[b]))
                    inside = (img[0] == other).nonzero()
                    if len(inside):  # the other sample's pixels form one full rectangle
                        (h0, w0), (h1, w1) = inside.min(0).values.tolist(), inside.max(0).values.tolist()
                        assert len(inside) == (h1 - h0 + 1) * (w1 - w0 + 1)
                        seen.add("cutmix")
                    else:
                        seen.add("plain")
                else:  # mixup: one blended value
                    assert len(vals) == 1
                    want = float(lam[b]) * own + (1.0 - float(lam[b])) * other
                    assert abs(vals.pop() - want) < 1e-5
                    seen.add("mixup")
    assert seen == {"plain", "cutmix", "mixup"}


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_cpu_loss(smoothing, reduction):
    from ringdp.nn import CrossEntropyLoss
    from ringdp.ops.mixup import MixedTarget

    B, C = 6, 5
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, C, generator=g, dtype=torch.float64).requires_grad_()
    y_a, y_b = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    loss = CrossEntropyLoss(label_smoothing=smoothing, reduction=reduction)(logits, MixedTarget(y_a, y_b, lam))
    rows = []
    for r in range(B):
        z = logits[r].tolist()
        lse = math.log(sum(math.exp(v) for v in z))
        q = [smoothing / C] * C
        q[int(y_a[r])] += (1 - smoothing) * float(lam[r])
        q[int(y_b[r])] += (1 - smoothing) * (1 - float(lam[r]))
        rows.append(sum(qc * (lse - zc) for qc, zc in zip(q, z)))
    want = {"mean": sum(rows) / B, "sum": sum(rows), "none": rows}[reduction]
    assert torch.allclose(loss, torch.tensor(want, dtype=torch.float64), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        CrossEntropyLoss(ignore_index=0)(logits, MixedTarget(y_a, y_b, lam))
    # the index-target path is untouched
    idx = CrossEntropyLoss(label_smoothing=smoothing, reduction=reduction)(logits, y_a)
    ref = torch.nn.functional.cross_entropy(logits, y_a, label_smoothing=smoothing, reduction=reduction)
    assert torch.equal(idx, ref)
