"""Mixup / CutMix on the GPU: the drawn records (invariants, determinism, the Beta law), the image kernel against an
expectation composed with torch ops from the records it read, the mixed-target cross entropy against ATen's
dense-target one and bit for bit against the index-target kernels at lam = 1 and 0, and the wiring: a vit_tiny
step, a captured training step whose mix advances with the replays, arguments and errors."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixup_common as mc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SNAPS = [(1234, 1), (2 ** 63 + 2 ** 40 + 7, 2 ** 32 + 5)]  # the second: high bits set in the seed and in the step


def _snap(seed, step):
    """A snapshot tensor as rng_tick would write it: (seed, step) as the int64 views of the u64 values."""
    s = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed, step)]
    return torch.tensor(s, dtype=torch.int64, device=DEV)


def _draw(seed, step, R, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5):
    from ringdp._native import C

    rec = C.mix_draw(_snap(seed, step), R, H, W, mixup_alpha, cutmix_alpha, prob, switch_prob)
    assert rec.shape == (R, 8) and rec.dtype == torch.int32
    return rec


def _ulp_bf16(v):
    """One bf16 ulp at the magnitude of the fp64 values ``v`` (8 significand bits): test_dropout_gpu's definition."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


# ------------------------------------------------------------------------------------------------ 1. records
@pytest.mark.parametrize("seed,step", SNAPS, ids=["low", "high"])
@pytest.mark.parametrize("H,W", [(7, 9), (32, 32), (224, 224)])
@pytest.mark.parametrize("mode", ["batch", "elem"])
def test_records(mode, H, W, seed, step):
    R = 1 if mode == "batch" else 300  # 300 records: more than one workgroup of the draw kernel
    kinds = set()
    for k in range(8 if mode == "batch" else 1):  # batch mode has one record per draw: look at eight steps
        rec = _draw(seed, step + k, R, H, W, prob=0.8)
        kinds |= set(mc.check_records(rec.cpu().numpy(), H, W)["kind"].tolist())
        assert torch.equal(rec, _draw(seed, step + k, R, H, W, prob=0.8))  # a function of the snapshot alone
    assert mode == "batch" or kinds == {0, 1, 2}
    a, b = _draw(seed, step, R, H, W), _draw(seed, step + 1, R, H, W)
    assert not torch.equal(a, b)
    assert not torch.equal(a, _draw(seed + 1, step, R, H, W))
    for kw, kind in ((dict(prob=0.0), 0), (dict(switch_prob=0.0), 1), (dict(switch_prob=1.0), 2),
                     (dict(cutmix_alpha=0.0), 1), (dict(mixup_alpha=0.0), 2)):
        f = mc.check_records(_draw(seed, step, max(R, 16), H, W, **kw).cpu().numpy(), H, W)
        assert np.all(f["kind"] == kind), (kw, f["kind"])


# ------------------------------------------------------------------------------------------------ 2. the law
@pytest.mark.parametrize("alpha", [0.8, 1.0, 2.0])
def test_beta_law(alpha):
    """Two-sample Kolmogorov-Smirnov distance between 8192 device draws and 2^20 numpy draws of Beta(alpha, alpha),
    against the 0.1 % critical value 1.95 * sqrt((n + m) / (n * m)) = 0.0216."""
    n, m = 8192, 2 ** 20
    f = mc.check_records(_draw(99, 1, n, 32, 32, mixup_alpha=alpha, cutmix_alpha=0.0).cpu().numpy(), 32, 32)
    assert np.all(f["kind"] == 1)
    d = mc.ks_distance(f["lam"], np.random.default_rng(0).beta(alpha, alpha, m))
    bound = 1.95 * math.sqrt((n + m) / (n * m))
    print(f"alpha={alpha}: KS distance {d:.4f} (bound {bound:.4f})")
    assert d < bound, (alpha, d, bound)


def test_decision_shares_and_centres():
    n, H, W = 8192, 32, 48
    sd = 5 * math.sqrt(0.25 / n)
    f = mc.check_records(_draw(5, 2, n, H, W, prob=0.5).cpu().numpy(), H, W)
    assert abs(float((f["kind"] != 0).mean()) - 0.5) < sd
    f = mc.check_records(_draw(5, 3, n, H, W, switch_prob=0.5).cpu().numpy(), H, W)
    assert np.all(f["kind"] != 0) and abs(float((f["kind"] == 2).mean()) - 0.5) < sd
    f = mc.check_records(_draw(5, 4, n, H, W, mixup_alpha=0.0).cpu().numpy(), H, W)
    cy, cx = (f["y0"] + f["y1"]) / 2, (f["x0"] + f["x1"]) / 2
    for c, size in ((cy, H), (cx, W)):
        assert (c < size / 2).mean() > 0.3 and (c > size / 2).mean() > 0.3
    assert f["lam"].std() > 0.1 and not np.array_equal(f["y0"], f["x0"])


# ------------------------------------------------------------------------------------------------ 3. images
def _images(shape, dtype, channels_last):
    """|values| in [0.5, 2] with a sign that depends on the position only, so a sample and its partner agree in
    sign and lam * a + (1 - lam) * b does not cancel (then one rounding of (1 - lam) * b and one of the sum stay
    within one ulp of the result); image row 0 is the same in every sample: a == b there."""
    g = torch.Generator(device=DEV).manual_seed(sum(shape))
    mag = torch.rand(shape, device=DEV, generator=g) * 1.5 + 0.5
    sign = (torch.randint(0, 2, shape[1:], device=DEV, generator=g) * 2 - 1).expand(shape)
    x = (mag * sign).to(dtype)
    x[:, :, 0, :] = x[0, :, 0, :]
    y = torch.randperm(shape[0], device=DEV, generator=g) * 3 + 1
    return (x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()), y


def _records_for(mode, B, H, W):
    """Drawn records with hand-made ones among them: an empty box, the whole image, and a box whose x edges fall
    inside a 16-byte vector.  Batch mode gets one of each kind per call."""
    hand = [mc.make_record(float(mc.box_lam(1, H, 1, W - 2, H, W)), 2, (1, H, 1, W - 2), 0.5),
            mc.make_record(0.3, 1),
            mc.make_record(1.0, 2, (0, 0, 0, 0), 0.99),
            mc.make_record(0.0, 2, (0, H, 0, W), 0.0),
            mc.make_record(1.0, 0)]
    if mode == "batch":
        drawn = [_draw(77, s, 1, H, W, **kw).cpu().numpy()[0]
                 for s, kw in ((1, dict(cutmix_alpha=0.0)), (2, dict(mixup_alpha=0.0)))]
        return [np.stack([r]) for r in hand + drawn]
    made = [np.stack([hand[(b + s) % len(hand)] for b in range(B)]) for s in (0, 2)]
    return made + [_draw(77, 3, B, H, W, prob=0.8).cpu().numpy(), _draw(78, 4, B, H, W).cpu().numpy()]


IMAGE_SHAPES = [(5, 3, 7, 9), (4, 3, 32, 32), (3, 3, 224, 224), (4, 4, 4, 6)]


def _check_images(shape, dtype, channels_last, mode):
    from ringdp._native import C

    B, _, H, W = shape
    x, y = _images(shape, dtype, channels_last)
    keep = x.clone()
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    for rec in _records_for(mode, B, H, W):
        out, y_b = C.mix_images(x, y, torch.from_numpy(rec).to(DEV))
        assert out.dtype == dtype and out.shape == x.shape and out.stride() == x.stride()
        assert out.data_ptr() != x.data_ptr() and torch.equal(y_b, y.flip(0))
        kind, copied, blended = mc.expected_mix(x, rec)
        same = out.view(bits) == copied.view(bits)
        plain = kind != 1
        assert bool(same[plain].all()), (rec, int((~same[plain]).sum()))
        if bool((kind == 1).any()):
            err = (out.double() - blended).abs()[~plain]
            tol = _ulp_bf16(blended)[~plain] if dtype == torch.bfloat16 else blended.abs()[~plain] * 2.0 ** -23
            assert bool((err <= tol).all()), float((err / tol).max())
            equal = (x == x.flip(0))[~plain]
            assert bool(equal.any()) and bool(same[~plain][equal].all())  # a == b: exact (copied is x there)
    assert torch.equal(x.view(bits), keep.view(bits))


@pytest.mark.parametrize("mode", ["batch", "elem"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", IMAGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_images(shape, dtype, channels_last, mode):
    """(5, 3, 7, 9): an odd batch whose samples are no whole 16-byte vectors (one element per thread);
    (4, 4, 4, 6): 16-byte vectors that run over the end of an image row."""
    _check_images(shape, dtype, channels_last, mode)


@pytest.mark.parametrize("mode", ["batch", "elem"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_images_grid_stride(channels_last, mode):
    """602112 vectors: more than the 2048 x 256 threads of the capped grid cover in one pass."""
    _check_images((32, 3, 224, 224), torch.bfloat16, channels_last, mode)


# ------------------------------------------------------------------------------------------------ 4. loss
def _lam_variants(B):
    g = torch.Generator(device=DEV).manual_seed(B)
    rec = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    rec.view(torch.float32)[:, 0] = torch.rand(B, device=DEV, generator=g)
    rec[:, 1:] = 7  # the words next to lam must not matter
    view = rec.view(torch.float32)[:, 0]
    assert view.stride(0) == 8
    return {"stride0": torch.full((1,), 0.3, device=DEV), "stride1": torch.rand(B, device=DEV, generator=g),
            "stride8": view}


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B,C", [(1, 10), (100, 10), (4097, 10), (33, 1000)])
def test_mixed_cross_entropy(B, C, smoothing):
    """Against ATen's dense-target cross entropy in fp32 at test_cross_entropy's tolerances; at lam = 1 (lam = 0)
    bit for bit the index-target kernels on y_a (y_b); two runs bit for bit alike."""
    from ringdp.ops.loss import _CrossEntropy
    from ringdp.ops.mixup import MixedTarget, mixed_cross_entropy

    g = torch.Generator(device=DEV).manual_seed(B + C)
    logits = torch.randn(B, C, device=DEV, generator=g) * 3
    y_a = torch.randint(0, C, (B,), device=DEV, generator=g)
    y_b = torch.randint(0, C, (B,), device=DEV, generator=g)

    def run(fn, reduction):
        z = logits.clone().requires_grad_()
        loss = fn(z)
        seed = torch.rand(loss.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) + 0.5
        (dz,) = torch.autograd.grad(loss, z, seed)
        return loss.detach(), dz

    for reduction in ("mean", "sum", "none"):
        for name, lam in _lam_variants(B).items():
            t = MixedTarget(y_a, y_b, lam)
            loss, dz = run(lambda z: mixed_cross_entropy(z, t, smoothing, reduction), reduction)
            want, dwant = run(lambda z: F.cross_entropy(z, t.dense(C), label_smoothing=smoothing,
                                                        reduction=reduction), reduction)
            assert loss.shape == want.shape
            torch.testing.assert_close(loss, want, rtol=1e-5, atol=1e-5, msg=lambda m: f"{name} {reduction}: {m}")
            torch.testing.assert_close(dz, dwant, rtol=1e-5, atol=1e-6, msg=lambda m: f"{name} {reduction}: {m}")
            again, dagain = run(lambda z: mixed_cross_entropy(z, t, smoothing, reduction), reduction)
            assert torch.equal(loss, again) and torch.equal(dz, dagain)
        for value, labels in ((1.0, y_a), (0.0, y_b)):
            index = run(lambda z: _CrossEntropy.apply(z, labels, -100, smoothing, reduction), reduction)
            for lam in (torch.full((1,), value, device=DEV), torch.full((B,), value, device=DEV)):
                mixed = run(lambda z: mixed_cross_entropy(z, MixedTarget(y_a, y_b, lam), smoothing, reduction),
                            reduction)
                assert torch.equal(mixed[0], index[0]) and torch.equal(mixed[1], index[1]), (value, reduction)


# ------------------------------------------------------------------------------------------------ wiring
def _tiny():
    from ringdp.models import vit_tiny

    torch.manual_seed(0)
    model = vit_tiny().cuda().train()
    torch.nn.init.normal_(model.heads.head.weight, std=0.5)  # the zero-initialised head hides the encoder
    return model


def test_vit_tiny_step():
    """One eager step through Mixup and CrossEntropyLoss against the same model fed the same mixed batch with
    ATen's dense-target cross entropy on its logits.  Gates of test_dropout_gpu's block parity test: 1e-2 on the
    output (here the loss), 2e-2 relative L2 on every gradient."""
    import ringdp.random as rr
    from ringdp.data import Mixup
    from ringdp.nn import CrossEntropyLoss

    model = _tiny()
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(16, 3, 32, 32, device=DEV, generator=g)
    y = torch.randint(0, 10, (16,), device=DEV, generator=g)
    mix = Mixup(0.8, 1.0)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    for seed in (7, 8):
        rr.manual_seed(seed, DEV)
        xm, target = mix(x, y)
        assert rr.get_rng_state(DEV) == (seed, 1) and not torch.equal(xm, x)
        model.zero_grad(set_to_none=True)
        loss = crit(model(xm), target)
        loss.backward()
        mine = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        want = F.cross_entropy(model(xm).float(), target.dense(10), label_smoothing=0.1)
        want.backward()
        loss, want = float(loss.detach()), float(want.detach())
        assert abs(loss - want) < 1e-2 * abs(want), (loss, want)
        for n, p in model.named_parameters():
            err = float((mine[n] - p.grad).float().norm() / p.grad.float().norm().clamp_min(1e-30))
            assert err < 2e-2, (n, err)


def test_captured_training_step():
    """Mixup + forward + backward + AdamW replayed from one hipGraph: lam and the box advance with the replays (the
    losses differ) and a restored generator state brings the same losses back bit for bit.  lr = 0 keeps the
    weights, so the loss depends on the mix alone."""
    import ringdp
    import ringdp.random as rr
    from ringdp.data import Mixup
    from ringdp.nn import CrossEntropyLoss
    from ringdp.utils.graph import StepGraph

    model = _tiny()
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(16, 3, 32, 32, device=DEV, generator=g)
    y = torch.randint(0, 10, (16,), device=DEV, generator=g)
    opt = ringdp.optim.AdamW(model.parameters(), lr=torch.zeros((), device=DEV), weight_decay=1e-2)
    mix = Mixup(0.8, 1.0)
    crit = CrossEntropyLoss(label_smoothing=0.1)
    seed_grad = torch.ones((), device=DEV)

    def step_fn():
        xm, target = mix(x, y)
        loss = crit(model(xm), target)
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


def test_arguments_and_errors():
    import ringdp.random as rr
    from ringdp._native import C
    from ringdp.data import Mixup
    from ringdp.nn import CrossEntropyLoss
    from ringdp.ops.mixup import MixedTarget, mix_batch

    x = torch.ones(4, 3, 8, 8, device=DEV)
    y = torch.arange(4, device=DEV)
    rr.manual_seed(5, DEV)
    # both alphas 0, or eval: the input itself, lam = 1, nothing drawn or launched
    for mod in (Mixup(0.0, 0.0), Mixup(0.8, 1.0).eval()):
        out, t = mod(x, y)
        assert out is x and t.y_a is y and torch.equal(t.lam, torch.ones(1, device=DEV))
    assert rr.get_rng_state(DEV) == (5, 0)
    out, t = Mixup(0.8, 1.0, mode="elem")(x, y)
    assert rr.get_rng_state(DEV) == (5, 1) and t.lam.shape == (4,) and t.lam.stride(0) == 8
    assert torch.equal(t.y_b, y.flip(0))
    logits = torch.zeros(4, 10, device=DEV)
    with pytest.raises(ValueError):
        CrossEntropyLoss(ignore_index=0)(logits, t)
    for bad in (x.half(), x.double(), x.to(torch.uint8)):
        with pytest.raises(TypeError):
            Mixup(0.8, 1.0)(bad, y)
    rec = _draw(1, 1, 1, 8, 8)
    with pytest.raises(TypeError):
        mix_batch(x.half(), y, rec)
    with pytest.raises(RuntimeError):
        C.mix_images(x.half(), y, rec)
    with pytest.raises(RuntimeError):
        C.mix_images(x, y, rec.cpu())
    with pytest.raises(RuntimeError):
        C.mix_images(x, y, _draw(1, 1, 3, 8, 8))  # three records for four samples
    with pytest.raises(RuntimeError):
        C.mix_images(x, y[:3], rec)
    with pytest.raises(RuntimeError):
        C.mix_images(x[:, :, ::2], y, rec)  # neither NCHW nor channels-last
    with pytest.raises(RuntimeError):
        C.mix_draw(_snap(1, 1), 1, 8, 8, -1.0, 0.0, 1.0, 0.5)
    with pytest.raises(RuntimeError):
        C.cross_entropy_mix_fwd(logits, y, y, torch.ones(3, device=DEV), 0.0, 1)
    with pytest.raises(RuntimeError):
        C.cross_entropy_mix_fwd(logits, y, y[:3], torch.ones(1, device=DEV), 0.0, 1)
    # a strided x is made contiguous by mix_batch, and the mix carries no gradient
    xs = torch.ones(4, 3, 8, 16, device=DEV, requires_grad=True)
    out, _ = mix_batch(xs[:, :, :, ::2], y, rec)
    assert out.shape == (4, 3, 8, 8) and not out.requires_grad
    assert MixedTarget(y, y, torch.ones(1, device=DEV)).dense(4).equal(torch.eye(4, device=DEV))
