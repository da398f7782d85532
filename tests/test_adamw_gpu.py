"""ringdp.optim.AdamW / Adam and ringdp.nn.utils.clip_grad_norm_ on the GPU against the fp64 torch oracle
(tests/adamw_common.py: oracle, gate rtol 1e-5 / atol 1e-6, shapes)."""
import pytest
import torch

from adamw_common import GRAD_SCALES, HYPERS, SHAPES, Flat, Oracle, grads_for, leaves, set_grads, values

pytestmark = pytest.mark.gpu

DEV = "cuda"
MISALIGNED = SHAPES + [(33,)]  # the last one becomes a leaf made from base[1:34]: the scalar path


def _setup(flat):
    shapes = SHAPES if flat else MISALIGNED
    vals = values(shapes)
    ps = leaves(vals, DEV, misaligned_last=not flat)
    return shapes, vals, ps, (Flat(ps) if flat else None)


def _give(ps, lay, grads):
    if lay is not None:
        lay.set_grads([g.to(DEV) for g in grads])
    else:
        set_grads(ps, grads, misaligned_last=True)


@pytest.mark.parametrize("lr,wd", HYPERS)
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "multi"])
def test_parity(flat, decoupled, maximize, lr, wd):
    import ringdp

    shapes, vals, ps, lay = _setup(flat)
    cls = ringdp.optim.AdamW if decoupled else ringdp.optim.Adam
    opt = cls(ps, lr=lr, weight_decay=wd, maximize=maximize)
    ref = Oracle(vals, decoupled, lr=lr, weight_decay=wd, maximize=maximize)
    for step in range(6):
        grads = grads_for(shapes, step, GRAD_SCALES[step % 3])
        _give(ps, lay, grads)
        opt.step()
        ref.step(grads)
        ref.check(ps, opt, f"step {step}")
    assert opt.grad_norm is None
    for p in ps:
        st = opt.state[p]["step"]
        assert st.dim() == 0 and st.dtype == torch.float32 and st.is_cuda and float(st) == 6


@pytest.mark.parametrize("lr,wd", HYPERS)
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "multi"])
def test_fused_clipping(flat, decoupled, lr, wd):
    """max_grad_norm=1.0 with gradient scales above (10) and below (1e-3) the threshold: both clip branches."""
    import ringdp

    shapes, vals, ps, lay = _setup(flat)
    cls = ringdp.optim.AdamW if decoupled else ringdp.optim.Adam
    opt = cls(ps, lr=lr, weight_decay=wd, max_grad_norm=1.0)
    ref = Oracle(vals, decoupled, max_norm=1.0, lr=lr, weight_decay=wd)
    for step, scale in enumerate([10.0, 1e-3, 10.0, 1e-3, 1.0, 0.1, 10.0, 1e-3]):
        grads = grads_for(shapes, step, scale)
        _give(ps, lay, grads)
        before = [p.grad.clone() for p in ps]
        opt.step()
        ref.step(grads)
        assert (float(ref.norm) > 1.0) == (scale >= 0.1)
        ref.check_norm(opt.grad_norm)
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
        for p, b in zip(ps, before):
            assert torch.equal(p.grad, b), "the fused clip must leave p.grad untouched"
        ref.check(ps, opt, f"step {step}")


@pytest.mark.parametrize("scale", [10.0, 1e-3])
def test_clip_grad_norm(scale):
    from ringdp.nn.utils import clip_grad_norm_

    vals = values(MISALIGNED)
    ps = leaves(vals, DEV, misaligned_last=True)
    grads = grads_for(MISALIGNED, 0, scale)
    set_grads(ps, grads, misaligned_last=True)
    ref_ps = [v.double().clone().requires_grad_() for v in vals]
    for p, g in zip(ref_ps, grads):
        p.grad = g.double().clone()
    want = torch.nn.utils.clip_grad_norm_(ref_ps, 1.0)
    got = clip_grad_norm_(ps, 1.0)
    assert got.is_cuda and got.dim() == 0
    torch.testing.assert_close(got.cpu().double(), want, rtol=1e-5, atol=0.0)
    for p, r in zip(ps, ref_ps):
        torch.testing.assert_close(p.grad.cpu().double().reshape(-1), r.grad.reshape(-1), rtol=1e-5, atol=1e-6)
    # determinism: identical gradients -> bitwise-equal norms, from two separate calls
    norms = []
    for _ in range(2):
        set_grads(ps, grads, misaligned_last=True)
        norms.append(clip_grad_norm_(ps, 1.0))
    assert norms[0].data_ptr() != norms[1].data_ptr()
    assert torch.equal(norms[0], norms[1]) and torch.equal(norms[0], got)


def test_clip_grad_norm_unsupported():
    from ringdp.nn.utils import clip_grad_norm_

    p = torch.randn(8, device=DEV, requires_grad=True)
    p.grad = torch.randn(8, device=DEV)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(NotImplementedError):
        clip_grad_norm_([p], 1.0, error_if_nonfinite=True)


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "multi"])
def test_graph_replay(flat):
    """Three warm-up steps, then 5 replays with new gradients and a changed lr before each: the step counter and
    the bias corrections must advance inside the graph, and lr must be read from the device."""
    import ringdp
    from ringdp.utils.graph import StepGraph

    shapes, vals, ps, lay = _setup(flat)
    lr = torch.tensor(1e-2, device=DEV)
    opt = ringdp.optim.AdamW(ps, lr=lr, weight_decay=1e-2, max_grad_norm=1.0)
    ref = Oracle(vals, True, max_norm=1.0, lr=1e-2, weight_decay=1e-2)
    static = [torch.zeros(s, device=DEV) for s in shapes]
    _give(ps, lay, [torch.zeros(s) for s in shapes])  # the gradient tensors the captured step writes into

    def step_fn():
        for p, g in zip(ps, static):
            p.grad.copy_(g.view_as(p.grad))
        opt.step()

    def feed(grads, lr_val):
        for s, g in zip(static, grads):
            s.copy_(g)
        lr.fill_(lr_val)
        ref.opt.param_groups[0]["lr"] = lr_val

    grads = grads_for(shapes, 0, 10.0)
    feed(grads, 1e-2)
    graph = StepGraph(step_fn, warmup=3).capture()
    for _ in range(3):
        ref.step(grads)
    for k, (scale, lr_val) in enumerate(zip([1e-3, 10.0, 1.0, 0.1, 10.0], [3e-2, 1e-3, 1e-2, 3e-2, 1e-3])):
        grads = grads_for(shapes, 1 + k, scale)
        feed(grads, lr_val)
        graph.replay()
        ref.step(grads)
        ref.check_norm(opt.grad_norm)
    torch.cuda.synchronize()
    ref.check(ps, opt, "after 3 warm-up steps and 5 replays")
    for p in ps:
        assert float(opt.state[p]["step"]) == 8


def test_two_groups_vit_tiny_shapes(monkeypatch):
    """Two param groups (different lr and weight decay) over vit_tiny's parameter shapes, one shared clip norm, and
    the launch bound 2 + G counted at the extension's entry points."""
    import ringdp
    from ringdp.models import vit_tiny
    from ringdp.optim import adamw as mod

    shapes = [tuple(p.shape) for p in vit_tiny(num_classes=10).parameters()]
    vals = values(shapes)
    ps = leaves(vals, DEV)
    decay = [i for i, s in enumerate(shapes) if len(s) >= 2]
    no_decay = [i for i, s in enumerate(shapes) if len(s) < 2]
    assert decay and no_decay
    groups = [(decay, dict(lr=1e-2, weight_decay=5e-2)), (no_decay, dict(lr=3e-2, weight_decay=0.0))]
    opt = ringdp.optim.AdamW([dict(params=[ps[i] for i in idx], **o) for idx, o in groups], max_grad_norm=1.0)
    ref = Oracle(vals, True, max_norm=1.0, groups=groups)

    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(ringdp._C, name)
            if not callable(fn) or isinstance(fn, type):
                return fn

            def wrapped(*a, **k):
                calls.append(name)
                return fn(*a, **k)

            return wrapped

    monkeypatch.setattr(mod, "C", Counting())
    launches = {"grad_sumsq_run", "adam_prepare_run", "adam_update_run", "adam_update_flat", "grad_scale_run"}
    for step, scale in enumerate([10.0, 1e-3, 1.0, 10.0, 0.1, 1e-3]):
        grads = grads_for(shapes, step, scale)
        if step == 0:
            set_grads(ps, grads)
        else:  # written in place, as a training loop's backward does: the addresses the table is keyed on stay
            for p, g in zip(ps, grads):
                p.grad.copy_(g)
        calls.clear()
        opt.step()
        got = [c for c in calls if c in launches]
        assert sorted(got) == ["adam_prepare_run", "adam_update_run", "adam_update_run", "grad_sumsq_run"], calls
        assert len(got) <= 2 + len(groups)
        if step > 0:
            assert "adam_table_build" not in calls, "the table must be cached once it exists"
        ref.step(grads)
        ref.check_norm(opt.grad_norm)
        ref.check(ps, opt, f"step {step}")
    # without clipping: 1 + G
    opt.max_grad_norm = None
    set_grads(ps, grads_for(shapes, 9, 1.0))
    calls.clear()
    opt.step()
    assert sorted(c for c in calls if c in launches) == ["adam_prepare_run", "adam_update_run", "adam_update_run"]


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "multi"])
def test_convnet_pack_invalidation(flat):
    """The raw kernels change the ConvNet's weights without bumping their versions: after a step the packed bf16
    fragments must be rebuilt, exactly as after an explicit invalidate_pack."""
    import ringdp
    from ringdp.models import ConvNet
    from ringdp.nn import CrossEntropyLoss
    from ringdp.ops.convnet import invalidate_pack

    torch.manual_seed(3)
    model = ConvNet().cuda()
    ps = list(model.parameters())
    lay = Flat(ps) if flat else None
    opt = ringdp.optim.AdamW(ps, lr=1e-2, weight_decay=1e-2)
    crit = CrossEntropyLoss()
    x, y = ringdp._C.synth_u8_images(8, 28, 28, 10, 0, torch.device("cuda", 0))
    for _ in range(3):
        loss = crit(model(x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if lay is not None:
            lay.set_grads([p.grad for p in ps])
        opt.step()
    out = model(x).detach().clone()
    invalidate_pack(model)
    want = model(x).detach().clone()
    assert torch.equal(out, want)
    # and the weights did move: the forward differs from one on the initial weights
    torch.manual_seed(3)
    fresh = ConvNet().cuda()
    assert not torch.equal(fresh(x).detach(), want)


@pytest.mark.parametrize("to_torch", [True, False], ids=["ringdp_to_torch", "torch_to_ringdp"])
def test_state_dict_round_trip(to_torch):
    """3 steps with one optimizer, its state_dict loaded into the other, 2 more steps: within the gate of the fp64
    oracle that ran all 5."""
    import ringdp

    vals = values(SHAPES)
    kw = dict(lr=1e-2, weight_decay=1e-2)
    ref = Oracle(vals, True, **kw)
    ps = leaves(vals, DEV)
    first_cls, second_cls = ((ringdp.optim.AdamW, torch.optim.AdamW) if to_torch
                             else (torch.optim.AdamW, ringdp.optim.AdamW))
    first = first_cls(ps, **kw)
    for step in range(3):
        grads = grads_for(SHAPES, step, GRAD_SCALES[step % 3])
        set_grads(ps, grads)
        first.step()
        ref.step(grads)
    second = second_cls(ps, **kw)
    second.load_state_dict(first.state_dict())
    for step in range(3, 5):
        grads = grads_for(SHAPES, step, GRAD_SCALES[step % 3])
        set_grads(ps, grads)
        second.step()
        ref.step(grads)
    ref.check(ps, second, "after the load")
    for p in ps:
        assert float(second.state[p]["step"]) == 5
    if not to_torch:
        steps = {second.state[p]["step"].data_ptr() for p in ps}
        assert len(steps) == 1, "one counter shared by the parameters of a group"
        assert all(second.state[p]["step"].is_cuda for p in ps)
