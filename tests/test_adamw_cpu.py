"""ringdp.optim.AdamW / Adam on the CPU path: parity with the fp64 torch oracle (tests/adamw_common.py), argument
validation, state_dict round trips with torch, and checkpoint resume."""
import pytest
import torch

from adamw_common import GRAD_SCALES, HYPERS, Oracle, grads_for, leaves, set_grads, values

SHAPES = [(10, 64), (10,), (33,), (1,), (8, 4, 3, 3)]


@pytest.mark.parametrize("lr,wd", HYPERS)
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip"])
def test_cpu_parity(clip, decoupled, maximize, lr, wd):
    import ringdp

    vals = values(SHAPES)
    ps = leaves(vals, "cpu")
    cls = ringdp.optim.AdamW if decoupled else ringdp.optim.Adam
    opt = cls(ps, lr=lr, weight_decay=wd, maximize=maximize, max_grad_norm=clip)
    ref = Oracle(vals, decoupled, max_norm=clip, lr=lr, weight_decay=wd, maximize=maximize)
    for step, scale in enumerate([10.0, 1e-3] + GRAD_SCALES * 2):
        grads = grads_for(SHAPES, step, scale)
        set_grads(ps, grads)
        before = [p.grad.clone() for p in ps]
        opt.step()
        ref.step(grads)
        if clip is not None:
            ref.check_norm(opt.grad_norm)
            assert all(torch.equal(p.grad, b) for p, b in zip(ps, before))
        ref.check(ps, opt, f"step {step}")
    st = opt.state[ps[0]]["step"]
    assert st.dim() == 0 and st.dtype == torch.float32 and float(st) == 8


def test_exports_and_defaults():
    import ringdp
    from ringdp.optim import SGD, Adam, AdamW  # noqa: F401

    p = torch.zeros(3, requires_grad=True)
    assert AdamW([p]).defaults["weight_decay"] == 1e-2 and AdamW([p]).defaults["decoupled_weight_decay"] is True
    assert Adam([p]).defaults["weight_decay"] == 0.0 and Adam([p]).defaults["decoupled_weight_decay"] is False
    assert issubclass(AdamW, torch.optim.Optimizer)
    # foreach / capturable / fused are accepted and ignored
    AdamW([p], foreach=True, capturable=True, fused=False)
    assert ringdp.nn.utils.clip_grad_norm_ is not None


@pytest.mark.parametrize("kw,exc", [
    (dict(lr=-1.0), ValueError),
    (dict(eps=-1e-8), ValueError),
    (dict(betas=(1.0, 0.999)), ValueError),
    (dict(betas=(0.9, -0.1)), ValueError),
    (dict(weight_decay=-1e-2), ValueError),
    (dict(max_grad_norm=0.0), ValueError),
    (dict(max_grad_norm=-1.0), ValueError),
    (dict(amsgrad=True), NotImplementedError),
    (dict(differentiable=True), NotImplementedError),
])
@pytest.mark.parametrize("name", ["AdamW", "Adam"])
def test_argument_validation(name, kw, exc):
    import ringdp

    p = torch.zeros(3, requires_grad=True)
    with pytest.raises(exc):
        getattr(ringdp.optim, name)([p], **kw)


def test_native_ops_fail_loudly_on_bad_input():
    """The GPU entry points take GPU fp32 tensors only: no quiet fall-back for anything else."""
    import ringdp

    C = ringdp._C
    t = torch.zeros(8)
    h = C.AdamHyper()
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.adam_table_build([t], [t], [t], [t], [1])
    with pytest.raises(RuntimeError, match="no tensors"):
        C.adam_table_build([], [], [], [], [])
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.adam_update_flat(t, t, t, t, t, 0, h)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.adam_prepare_run(t, None, 0, 0.0, [], [], [])
    with pytest.raises(RuntimeError, match="at most"):
        C.adam_prepare_run(t, None, 0, 0.0, [t] * 33, [None] * 33, [h] * 33)


def test_clip_grad_norm_cpu_defers_to_torch():
    from ringdp.nn.utils import clip_grad_norm_

    vals = values(SHAPES)
    ps, ref = leaves(vals, "cpu"), leaves(vals, "cpu")
    grads = grads_for(SHAPES, 0, 10.0)
    set_grads(ps, grads)
    set_grads(ref, grads)
    for norm_type in (2.0, 1.0, float("inf")):
        got = clip_grad_norm_(ps, 1.0, norm_type=norm_type)
        want = torch.nn.utils.clip_grad_norm_(ref, 1.0, norm_type=norm_type)
        assert torch.equal(got, want)
        assert all(torch.equal(a.grad, b.grad) for a, b in zip(ps, ref))


@pytest.mark.parametrize("to_torch", [True, False], ids=["ringdp_to_torch", "torch_to_ringdp"])
def test_state_dict_round_trip(to_torch):
    import ringdp

    vals = values(SHAPES)
    kw = dict(lr=1e-2, weight_decay=1e-2)
    ref = Oracle(vals, True, **kw)
    ps = leaves(vals, "cpu")
    first_cls, second_cls = ((ringdp.optim.AdamW, torch.optim.AdamW) if to_torch
                             else (torch.optim.AdamW, ringdp.optim.AdamW))
    first = first_cls(ps, **kw)
    for step in range(3):
        grads = grads_for(SHAPES, step, GRAD_SCALES[step % 3])
        set_grads(ps, grads)
        first.step()
        ref.step(grads)
    sd = first.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    second = second_cls(ps, **kw)
    second.load_state_dict(sd)
    for step in range(3, 5):
        grads = grads_for(SHAPES, step, GRAD_SCALES[step % 3])
        set_grads(ps, grads)
        second.step()
        ref.step(grads)
    ref.check(ps, second, "after the load")
    assert all(float(second.state[p]["step"]) == 5 for p in ps)


def test_load_rejects_unequal_steps():
    import ringdp

    ps = leaves(values(SHAPES), "cpu")
    opt = ringdp.optim.AdamW(ps)
    set_grads(ps, grads_for(SHAPES, 0, 1.0))
    opt.step()
    sd = opt.state_dict()
    sd["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="one step counter per parameter group"):
        ringdp.optim.AdamW(ps).load_state_dict(sd)


def test_checkpoint_resume(tmp_path):
    """2 steps, save, 2 more == a fresh model and optimizer resuming from the file."""
    import ringdp
    from ringdp.utils import checkpoint

    def make():
        torch.manual_seed(3)
        m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
        return m, ringdp.optim.AdamW(m.parameters(), lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0)

    def train(m, opt, steps):
        for s in steps:
            g = torch.Generator().manual_seed(s)
            x = torch.randn(16, 7, generator=g) * 10
            opt.zero_grad(set_to_none=True)
            m(x).square().mean().backward()
            opt.step()

    m1, o1 = make()
    train(m1, o1, [0, 1])
    path = str(tmp_path / "ck.pt")
    checkpoint.save(path, m1, o1, step=2)
    train(m1, o1, [2, 3])

    m2, o2 = make()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)  # the file must restore them
    meta = checkpoint.load(path, m2, o2)
    assert meta["step"] == 2
    train(m2, o2, [2, 3])
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    for a, b in zip(m1.parameters(), m2.parameters()):
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(o1.state[a][name], o2.state[b][name])
    assert float(o2.state[next(m2.parameters())]["step"]) == 4
