"""ringdp.optim.lr_scheduler and ringdp.utils.ModelEma on the GPU: the device-side schedules against the fp64 closed
form and torch's schedulers, the optimizers following the written lr, the EMA kernels against the element contract,
the shadow's forward, and the whole step captured by StepGraph (tests/sched_ema_common.py: closed forms, gates)."""
import functools

import pytest
import torch

import sched_ema_common as sc
from adamw_common import ATOL, RTOL, SHAPES, Flat, Oracle, grads_for, leaves, set_grads, values

pytestmark = pytest.mark.gpu

DEV = "cuda"
MISALIGNED = SHAPES + [(33,)]  # the last one becomes a leaf made from base[1:34]: the scalar path


def _opt(bases=sc.BASES, lrs=None):
    import ringdp

    ps = [torch.zeros(3, device=DEV, requires_grad=True) for _ in bases]
    return ringdp.optim.SGD([dict(params=[p], lr=b if lrs is None else lrs[i])
                             for i, (p, b) in enumerate(zip(ps, bases))])


def _run(sched, opt, steps):
    """lr of every group before each of ``steps`` scheduler steps, read back once at the end: fp32 [steps, groups]."""
    rows = []
    for _ in range(steps):
        rows.append(torch.stack([g["lr"] for g in opt.param_groups]))
        sched.step()
    return torch.stack(rows).cpu()


# ---------------------------------------------------------------------------------------------- schedule values
@pytest.mark.parametrize("period", sc.PERIODS)
@pytest.mark.parametrize("name", list(sc.KINDS))
def test_closed_form(name, period):
    differ = points = 0
    for W, a in sc.WARMUPS:
        opt = _opt()
        sched = sc.make_scheduler(name, opt, W, a, period)
        for g in opt.param_groups:
            lr = g["lr"]
            assert torch.is_tensor(lr) and lr.dim() == 0 and lr.dtype == torch.float32 and lr.is_cuda
        assert [g["initial_lr"] for g in opt.param_groups] == sc.BASES
        got = _run(sched, opt, sc.steps_for(period))
        worst, n = sc.ulp_report(got, sc.expected_lrs(name, W, a, period))
        differ, points = differ + n, points + got.numel()
        assert worst <= 1, (name, W, a, period, worst)
        assert sched.last_epoch == sc.steps_for(period)
    print(f"gpu schedule {name} period {period}: {differ} of {points} points differ from the closed form")


@pytest.mark.parametrize("name", sc.TORCH_NAMES)
def test_matches_torch_schedulers(name):
    opt = _opt()
    got = _run(sc.ringdp_for_torch(name, opt), opt, sc.TOTAL + 6).double()
    n = sc.torch_rows(name)
    # the device value is rounded to fp32 (6e-8), inside the rtol
    torch.testing.assert_close(got[:n], sc.torch_reference(name)[:n], rtol=1e-6, atol=0.0)


# ---------------------------------------------------------------------------------------------- plumbing
class SgdOracle:
    """fp64 torch.optim.SGD on CPU copies."""

    def __init__(self, vals, **kw):
        self.ps = [v.double().clone().requires_grad_() for v in vals]
        self.opt = torch.optim.SGD(self.ps, **kw)

    def step(self, grads):
        for p, g in zip(self.ps, grads):
            p.grad = g.double().clone().view_as(p)
        self.opt.step()

    def check(self, my_ps, my_opt, what=""):
        for i, (a, r) in enumerate(zip(my_ps, self.ps)):
            pairs = [("param", a.detach(), r.detach()),
                     ("momentum", my_opt.state[a]["momentum_buffer"], self.opt.state[r]["momentum_buffer"])]
            for name, x, y in pairs:
                torch.testing.assert_close(x.detach().cpu().double().reshape(-1), y.reshape(-1), rtol=RTOL, atol=ATOL,
                                           msg=lambda m, i=i, name=name: f"{what} tensor {i} {name}: {m}")


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "multi"])
@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_optimizers_follow_the_schedule(which, flat):
    """8 scheduled steps (warmup 2, the cosine's end at 6, then the end point) against the fp64 oracle stepped with
    the closed-form lr."""
    import ringdp

    shapes = SHAPES if flat else MISALIGNED
    vals = values(shapes)
    ps = leaves(vals, DEV, misaligned_last=not flat)
    lay = Flat(ps) if flat else None
    base = 1e-2
    if which == "sgd":
        kw = dict(momentum=0.9, weight_decay=1e-4)
        opt, ref = ringdp.optim.SGD(ps, lr=base, **kw), SgdOracle(vals, lr=base, **kw)
    else:
        opt = ringdp.optim.AdamW(ps, lr=base, weight_decay=1e-2)
        ref = Oracle(vals, True, lr=base, weight_decay=1e-2)
    sched = ringdp.optim.lr_scheduler.WarmupCosineLR(opt, 6, 0.05, warmup_steps=2, warmup_start_factor=0.1)

    def f(k):
        if k < 2:
            return 0.1 + 0.9 * k / 2
        import math
        return 0.05 + 0.95 * (1 + math.cos(math.pi * min(k - 2, 4) / 4)) / 2

    for k in range(8):
        grads = grads_for(shapes, k, 1.0)
        if lay is not None:
            lay.set_grads([g.to(DEV) for g in grads])
        else:
            set_grads(ps, grads, misaligned_last=True)
        ref.opt.param_groups[0]["lr"] = float(torch.tensor(base * f(k), dtype=torch.float64).float())
        opt.step()
        sched.step()
        ref.step(grads)
        ref.check(ps, opt, f"step {k}")
    assert sched.last_epoch == 8
    assert sched.get_last_lr() == [float(torch.tensor(base * f(8), dtype=torch.float64).float())]


def test_existing_lr_tensor_is_kept():
    import ringdp

    p = torch.zeros(8, device=DEV, requires_grad=True)
    lr = torch.tensor(1e-2, device=DEV)
    addr = lr.data_ptr()
    opt = ringdp.optim.AdamW([p], lr=lr)
    sched = ringdp.optim.lr_scheduler.WarmupConstantLR(opt, warmup_steps=4, warmup_start_factor=0.5)
    assert opt.param_groups[0]["lr"] is lr and lr.data_ptr() == addr
    assert opt.param_groups[0]["initial_lr"] == float(torch.tensor(1e-2))
    base = float(torch.tensor(1e-2))
    assert float(lr) == float(torch.tensor(base * 0.5, dtype=torch.float64).float())  # lr(0) was written
    sched.step()
    assert opt.param_groups[0]["lr"] is lr and lr.data_ptr() == addr
    assert float(lr) == float(torch.tensor(base * (0.5 + 0.5 * 1 / 4), dtype=torch.float64).float())


def test_state_dict_round_trip():
    opt = _opt()
    a = sc.make_scheduler("cosine", opt, 3, 0.1, 3)
    _run(a, opt, 7)
    sd = a.state_dict()
    assert sd["last_epoch"] == 7 and isinstance(sd["last_epoch"], int)
    assert all(not torch.is_tensor(v) for v in sd["spec"].values()) and sd["base_lrs"] == sc.BASES
    now = torch.stack([g["lr"] for g in opt.param_groups]).cpu()
    rest = _run(a, opt, 5)
    opt2 = _opt(lrs=[0.5, 0.5])  # whatever lr the fresh optimizer was built with: the state brings the bases
    b = sc.make_scheduler("cosine", opt2, 3, 0.1, 3)
    counter, lrs = b._counter.data_ptr(), [g["lr"].data_ptr() for g in opt2.param_groups]
    b.load_state_dict(sd)
    assert b._counter.data_ptr() == counter and [g["lr"].data_ptr() for g in opt2.param_groups] == lrs
    assert b.last_epoch == 7
    assert torch.equal(torch.stack([g["lr"] for g in opt2.param_groups]).cpu(), now)
    assert torch.equal(_run(b, opt2, 5), rest)
    assert b.last_epoch == a.last_epoch == 12


def test_errors():
    import ringdp
    from ringdp.optim import lr_scheduler as L

    ps = [torch.zeros(2, device=DEV, requires_grad=True) for _ in range(33)]
    with pytest.raises(NotImplementedError, match="at most 32"):
        L.WarmupConstantLR(ringdp.optim.SGD([dict(params=[p]) for p in ps], lr=0.1))
    L.WarmupConstantLR(ringdp.optim.SGD([dict(params=[p]) for p in ps[:32]], lr=0.1))  # 32 are fine
    p = ps[0]
    for bad in (torch.tensor([1e-2], device=DEV), torch.tensor(1e-2, device=DEV, dtype=torch.float64),
                torch.tensor(1e-2)):
        with pytest.raises(ValueError, match="0-dim float32"):
            L.WarmupConstantLR(ringdp.optim.AdamW([p], lr=bad))
    with pytest.raises(ValueError, match="must exceed warmup_steps"):
        L.WarmupCosineLR(ringdp.optim.SGD([p], lr=0.1), 3, warmup_steps=3)
    with pytest.raises(ValueError, match="sorted"):
        L.WarmupMultiStepLR(ringdp.optim.SGD([p], lr=0.1), [9, 4])
    with pytest.raises(ValueError, match="at most 8"):
        L.WarmupMultiStepLR(ringdp.optim.SGD([p], lr=0.1), list(range(1, 10)))
    # the extension checks the same on its own
    C, spec = ringdp._C, ringdp._C.LrSchedSpec()
    n, t = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros((), device=DEV)
    spec.total_steps, spec.warmup_steps = 3, 3
    with pytest.raises(RuntimeError, match="must exceed warmup_steps"):
        C.lr_sched_run(n, spec, [0.1], [t], True)
    spec.total_steps, spec.milestones = 4, [9, 4]
    with pytest.raises(RuntimeError, match="sorted"):
        C.lr_sched_run(n, spec, [0.1], [t], True)
    spec.milestones = list(range(9))
    with pytest.raises(RuntimeError, match="at most 8"):
        C.lr_sched_run(n, spec, [0.1], [t], True)
    spec.milestones = []
    with pytest.raises(RuntimeError, match="between 1 and 32"):
        C.lr_sched_run(n, spec, [0.1] * 33, [torch.zeros((), device=DEV) for _ in range(33)], True)
    with pytest.raises(RuntimeError, match="0-dim"):
        C.lr_sched_run(n, spec, [0.1], [torch.zeros(1, device=DEV)], True)
    with pytest.raises(RuntimeError, match="expected dtype"):
        C.lr_sched_run(n, spec, [0.1], [t.double()], True)
    with pytest.raises(RuntimeError, match="expected dtype"):
        C.lr_sched_run(t, spec, [0.1], [t], True)
    assert int(n) == 0, "a rejected call launches nothing"


# ---------------------------------------------------------------------------------------------- EMA kernels
FORMS = ["flat", "multi", "multi_misaligned"]


def _ema_model(form):
    shapes = MISALIGNED if form == "multi_misaligned" else SHAPES
    ps = leaves(values(shapes), DEV, misaligned_last=form == "multi_misaligned")
    lay = Flat(ps) if form == "flat" else None
    model = sc.Bag(ps)
    if lay is not None:
        for p, t in zip(model.ps, ps):
            p._ringdp_flat = t._ringdp_flat
    return shapes, model


@functools.lru_cache(maxsize=None)
def _ema_run(form, decay, warmup):
    """K = 6 updates with changing parameters.  Per update: (shadow before, parameters, w, shadow after) on the
    CPU.  Computed once per case and shared."""
    from ringdp.utils import ModelEma

    shapes, model = _ema_model(form)
    ema = ModelEma(model, decay=decay, warmup=warmup)
    if form == "multi_misaligned":  # a misaligned shadow too: both pointers of the last chunk take the scalar loop
        e = ema.module.ps[-1]
        base = torch.zeros(e.numel() + 8, device=DEV)
        base[1:1 + e.numel()].copy_(e.data)
        e.data = base[1:1 + e.numel()]
        assert e.data_ptr() % 16 == 4 and model.ps[-1].data_ptr() % 16 == 4
    steps = []
    for k in range(6):
        with torch.no_grad():
            for p, v in zip(model.ps, values(shapes, seed=20 + k)):
                p.add_(v.to(DEV))
        before = [e.detach().cpu().clone() for e in ema.module.ps]
        ema.update()
        steps.append((before, [p.detach().cpu().clone() for p in model.ps], ema._w.cpu().clone(),
                      [e.detach().cpu().clone() for e in ema.module.ps]))
    assert int(ema.num_updates) == 6 and ema.num_updates.dtype == torch.int64 and ema.num_updates.is_cuda
    if form == "flat":
        plan = ema._plan
        assert len(plan[1]) == 1 and plan[2] is None, "one flat range, no table"
        sf = plan[1][0][0]
        for e, p in zip(ema.module.ps, model.ps):
            assert e.data_ptr() == sf.data_ptr() + p._ringdp_flat[2] * 4, "the shadow's parameters view its flat buffer"
    else:
        plan = ema._plan
        assert not plan[1] and plan[2].pair and plan[2].all_aligned == [form == "multi"]
    return steps


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.9, 0.9999])
@pytest.mark.parametrize("form", FORMS)
def test_ema_contract(form, decay, warmup):
    unequal = total = 0
    for k, (before, params, w, after) in enumerate(_ema_run(form, decay, warmup)):
        worst, _ = sc.ulp_report(w.reshape(1), sc.ema_weight(k + 1, decay, warmup).reshape(1))
        assert worst <= 1, f"update {k}: w = {float(w)}"
        for i, (e, p, got) in enumerate(zip(before, params, after)):
            worst, n = sc.ulp_report(got, sc.ema_contract(e, p, w))
            unequal, total = unequal + n, total + got.numel()
            assert worst <= 1, f"update {k} tensor {i}: {worst} ulp"
            assert got.numel() < 8 or not torch.equal(got, e), "the shadow must move"
    print(f"ema {form} decay {decay} warmup {warmup}: {unequal} of {total} elements differ from the fp64-emulated fma")


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_ema_flat_equals_multi(decay, warmup):
    flat, multi, mis = (_ema_run(f, decay, warmup) for f in FORMS)
    for (_, _, wa, a), (_, _, wb, b), (_, _, wc, c) in zip(flat, multi, mis):
        assert torch.equal(wa, wb) and torch.equal(wa, wc)
        for x, y, z in zip(a, b, c):  # the misaligned run has one more tensor at the end
            assert torch.equal(x, y) and torch.equal(x, z)


def test_ema_buffers_and_bf16():
    from ringdp.utils import ModelEma

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3)).to(DEV)
    ema = ModelEma(model, decay=0.5)
    with torch.no_grad():
        model[1].running_mean.fill_(2.0)
        model[1].num_batches_tracked.fill_(7)
    ema.update()
    assert torch.equal(ema.module[1].running_mean.cpu(), torch.full((3,), 1.0))  # the float buffer is averaged
    assert int(ema.module[1].num_batches_tracked) == 7                           # the integer buffer is copied
    with pytest.raises(NotImplementedError, match="float32"):
        ModelEma(torch.nn.Linear(4, 3).to(DEV).bfloat16())


def test_ema_state_dict_and_set():
    from ringdp.utils import ModelEma

    _, model = _ema_model("multi")
    ema = ModelEma(model, decay=0.9, warmup=True)
    for k in range(3):
        with torch.no_grad():
            for p, v in zip(model.ps, values(SHAPES, seed=30 + k)):
                p.add_(v.to(DEV))
        ema.update()
    sd = {k: v.clone() for k, v in ema.state_dict().items()}
    assert set(sd) == set(model.state_dict()) | {"num_updates"} and int(sd["num_updates"]) == 3
    other = ModelEma(model, decay=0.9, warmup=True)
    other.update()  # builds its table; the load must keep it
    ptrs, plan = [e.data_ptr() for e in other.module.ps], other._plan
    other.load_state_dict(sd)
    assert ptrs == [e.data_ptr() for e in other.module.ps], "the load writes in place"
    assert int(other.num_updates) == 3
    for a, b in zip(other.module.ps, ema.module.ps):
        assert torch.equal(a, b)
    ema.update()
    other.update()
    assert other._plan is plan
    assert int(other.num_updates) == 4 and torch.equal(other._w, ema._w)
    for a, b in zip(other.module.ps, ema.module.ps):
        assert torch.equal(a, b)
    ema.set(model)
    for a, b in zip(ema.module.ps, model.ps):
        assert torch.equal(a, b)


def test_ema_of_a_ddp_model_is_flat():
    """A ringdp DistributedDataParallel is unwrapped and its flattened parameter buffer found: the update is the
    flat launch, also after the bucket rebuild of the first iterations moved the buffer; every update within 1 ulp
    of the contract."""
    import ringdp
    import ringdp.distributed as dist
    from ringdp.models import ConvNet
    from ringdp.nn import CrossEntropyLoss
    from ringdp.parallel import DistributedDataParallel as DDP
    from ringdp.utils import ModelEma

    if not dist.is_initialized():
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1)
    try:
        torch.manual_seed(0)
        model = ConvNet().cuda()
        ddp = DDP(model, device_ids=[0])
        opt = ringdp.optim.SGD(ddp.parameters(), lr=1e-2, momentum=0.9)
        ema = ModelEma(ddp, decay=0.9, warmup=True)
        assert ema._source is model and not isinstance(ema.module, DDP)
        crit = CrossEntropyLoss()
        x, y = ringdp._C.synth_u8_images(8, 28, 28, 10, 0, torch.device("cuda", 0))
        for k in range(4):
            loss = crit(ddp(x), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            before = [e.detach().cpu().clone() for e in ema.module.parameters()]
            ema.update()
            _, flats, table = ema._plan
            assert len(flats) == 1 and table is None, "one flat launch"
            sf, fp = flats[0]
            assert fp is next(model.parameters())._ringdp_flat[0] and sf.numel() == fp.numel()
            for e, p, b in zip(ema.module.parameters(), model.parameters(), before):
                assert e.data_ptr() == sf.data_ptr() + p._ringdp_flat[2] * 4
                worst, _ = sc.ulp_report(e.detach().cpu(), sc.ema_contract(b, p.detach().cpu(), ema._w.cpu()))
                assert worst <= 1, (k, worst)
        assert int(ema.num_updates) == 4
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------- the shadow
@pytest.mark.parametrize("which", ["convnet", "vit_tiny"])
def test_shadow_forward(which):
    """The shadow after two updates computes what a fresh model loaded from its state dict computes, bit for bit:
    no stale packed fragments, no state shared with the source."""
    import ringdp
    from ringdp.models import ConvNet, vit_tiny
    from ringdp.utils import ModelEma

    torch.manual_seed(3)
    if which == "convnet":
        make = ConvNet
        x, _ = ringdp._C.synth_u8_images(8, 28, 28, 10, 0, torch.device("cuda", 0))
    else:
        make = vit_tiny
        x = torch.randn(4, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    model = make().to(DEV)
    if which == "vit_tiny":
        torch.nn.init.normal_(model.heads.head.weight, std=0.5)  # the zero-initialised head hides the encoder
    with torch.no_grad():
        model(x)  # the source has packed its fragments before it is copied
    ema = ModelEma(model, decay=0.9)
    assert not ema.module.training
    outs = []
    with torch.no_grad():
        outs.append(ema.module(x).clone())
        for k in range(2):
            for p in model.parameters():
                p.add_(0.05 * torch.randn_like(p))
            ema.update()
            outs.append(ema.module(x).clone())
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    sd = ema.state_dict()
    assert int(sd.pop("num_updates")) == 2
    fresh = make().to(DEV).eval()
    fresh.load_state_dict(sd)
    with torch.no_grad():
        want = fresh(x)
        assert torch.equal(outs[2], want)
        assert not torch.equal(model.eval()(x), want)
    if which == "convnet":
        from ringdp.ops.convnet import pack_states

        st = ema.module.conv1.__dict__["_ringdp_pack_state"]
        assert st is not model.conv1.__dict__["_ringdp_pack_state"] and st in pack_states()


# ---------------------------------------------------------------------------------------------- captured step
def test_captured_step(monkeypatch):
    """vit_tiny forward + backward, AdamW with clipping, the cosine schedule and the EMA update captured in one
    StepGraph: 3 warm-up steps and 5 replays against 8 eager calls of the same step function from the same state.
    lr and both counters must be bitwise equal.  Parameters and EMA weights are held to the standard of
    test_adamw_gpu.py::test_graph_replay, which is the optimizer gate (rtol 1e-5 / atol 1e-6), not bitwise."""
    import ringdp
    from ringdp.models import vit_tiny
    from ringdp.nn import CrossEntropyLoss
    from ringdp.optim import adamw as adamw_mod
    from ringdp.utils import ModelEma
    from ringdp.utils import ema as ema_mod
    from ringdp.utils.graph import StepGraph

    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(16, 3, 32, 32, device=DEV, generator=g)
    y = torch.randint(0, 10, (16,), device=DEV, generator=g)
    torch.manual_seed(0)
    init = vit_tiny().to(DEV)
    torch.nn.init.normal_(init.heads.head.weight, std=0.5)
    seed_grad = torch.ones((), device=DEV)

    def build():
        model = vit_tiny().to(DEV)
        model.load_state_dict(init.state_dict())
        model.train()
        opt = ringdp.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
        sched = ringdp.optim.lr_scheduler.WarmupCosineLR(opt, 7, 0.05, warmup_steps=2, warmup_start_factor=0.1)
        ema = ModelEma(model, decay=0.9, warmup=True)
        crit = CrossEntropyLoss()

        def step_fn():
            loss = crit(model(x), y)
            opt.zero_grad(set_to_none=False)
            loss.backward(seed_grad)
            opt.step()
            sched.step()
            ema.update()
            return loss

        return model, opt, sched, ema, step_fn

    model_e, opt_e, sched_e, ema_e, eager = build()
    for _ in range(8):
        eager()

    model, opt, sched, ema, step_fn = build()
    graph = StepGraph(step_fn, warmup=3).capture()
    # the capture itself launches nothing: 3 warm-up steps so far
    assert sched.last_epoch == 3 and int(ema.num_updates) == 3
    lr = opt.param_groups[0]["lr"]
    addrs = (lr.data_ptr(), sched._counter.data_ptr(), ema.num_updates.data_ptr(), ema._w.data_ptr())
    plans = (opt._plan, ema._plan)
    built = []
    for mod in (adamw_mod, ema_mod):
        real = mod.C

        class Counting:
            def __getattr__(self, name, real=real):
                fn = getattr(real, name)
                if name != "adam_table_build":
                    return fn
                return lambda *a, **k: (built.append(name), fn(*a, **k))[1]

        monkeypatch.setattr(mod, "C", Counting())
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem, "a replay allocates nothing"
    assert (opt._plan, ema._plan) == plans and opt._plan is plans[0] and ema._plan is plans[1]
    assert addrs == (lr.data_ptr(), sched._counter.data_ptr(), ema.num_updates.data_ptr(), ema._w.data_ptr())

    assert sched.last_epoch == sched_e.last_epoch == 8
    assert int(ema.num_updates) == int(ema_e.num_updates) == 8
    assert torch.equal(lr, opt_e.param_groups[0]["lr"])
    assert torch.equal(ema._w, ema_e._w)
    want_lr = torch.tensor(1e-3 * sc_cosine(8), dtype=torch.float64).float()
    assert sc.ulp_report(lr.cpu().reshape(1), want_lr.reshape(1))[0] <= 1
    bitwise = True
    for what, mine, theirs in (("param", model, model_e), ("ema", ema.module, ema_e.module)):
        for (name, a), (_, b) in zip(mine.named_parameters(), theirs.named_parameters()):
            bitwise = bitwise and torch.equal(a, b)
            torch.testing.assert_close(a.detach(), b.detach(), rtol=RTOL, atol=ATOL,
                                       msg=lambda m, what=what, name=name: f"{what} {name}: {m}")
    print(f"captured step: parameters and EMA weights bitwise equal to eager: {bitwise}")
    # an eager step after the replays finds every table as the capture left it: nothing is rebuilt or uploaded
    step_fn()
    assert built == [] and opt._plan is plans[0] and ema._plan is plans[1]
    assert sched.last_epoch == 9 and int(ema.num_updates) == 9


def sc_cosine(k):
    """The captured step's schedule: warmup 2 from 0.1, the cosine's end (0.05) at 7."""
    import math

    if k < 2:
        return 0.1 + 0.9 * k / 2
    return 0.05 + 0.95 * (1 + math.cos(math.pi * min(k - 2, 5) / 5)) / 2
