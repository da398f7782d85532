"""ringdp.optim.lr_scheduler and ringdp.utils.ModelEma on the CPU path: the schedules against the fp64 closed form
and torch's schedulers, the ``_foreach_lerp_`` EMA against fp64, state dicts, and argument validation
(tests/sched_ema_common.py: closed forms, cases, gates)."""
import pytest
import torch

import sched_ema_common as sc
from adamw_common import values

SHAPES = [(10, 64), (10,), (33,), (1,), (8, 4, 3, 3)]


def _opt(bases=sc.BASES, dtype=torch.float32):
    import ringdp

    ps = [torch.zeros(3, dtype=dtype, requires_grad=True) for _ in bases]
    return ringdp.optim.SGD([dict(params=[p], lr=b) for p, b in zip(ps, bases)])


def _run(sched, opt, steps):
    rows = []
    for _ in range(steps):
        rows.append([g["lr"] for g in opt.param_groups])
        assert all(isinstance(v, float) for v in rows[-1]), "the CPU path keeps group['lr'] a Python float"
        opt.step()
        sched.step()
    return rows


@pytest.mark.parametrize("period", sc.PERIODS)
@pytest.mark.parametrize("name", list(sc.KINDS))
def test_closed_form(name, period):
    differ = points = 0
    for W, a in sc.WARMUPS:
        opt = _opt()
        sched = sc.make_scheduler(name, opt, W, a, period)
        assert [g["initial_lr"] for g in opt.param_groups] == sc.BASES
        rows = _run(sched, opt, sc.steps_for(period))
        got = torch.tensor(rows, dtype=torch.float64).float()
        worst, n = sc.ulp_report(got, sc.expected_lrs(name, W, a, period))
        differ, points = differ + n, points + got.numel()
        assert worst <= 1, (name, W, a, period, worst)
        assert sched.last_epoch == sc.steps_for(period)
        assert sched.get_last_lr() == [g["lr"] for g in opt.param_groups]
    print(f"cpu schedule {name} period {period}: {differ} of {points} points differ from the closed form")


@pytest.mark.parametrize("name", sc.TORCH_NAMES)
def test_matches_torch_schedulers(name):
    opt = _opt(dtype=torch.float64)
    sched = sc.ringdp_for_torch(name, opt)
    got = torch.tensor(_run(sched, opt, sc.TOTAL + 6), dtype=torch.float64)
    n = sc.torch_rows(name)
    torch.testing.assert_close(got[:n], sc.torch_reference(name)[:n], rtol=1e-6, atol=0.0)


def test_past_the_end_stays():
    opt = _opt()
    sched = sc.make_scheduler("cosine", opt, 3, 0.1, 1)
    rows = _run(sched, opt, sc.TOTAL + 6)
    assert all(r == rows[sc.TOTAL] for r in rows[sc.TOTAL:])
    assert rows[sc.TOTAL] == [b * 0.05 for b in sc.BASES]


def test_state_dict_round_trip():
    opt = _opt()
    a = sc.make_scheduler("cosine", opt, 3, 0.1, 3)
    _run(a, opt, 7)
    sd = a.state_dict()
    assert sd["last_epoch"] == 7 and isinstance(sd["last_epoch"], int)
    assert all(not torch.is_tensor(v) for v in sd["spec"].values()) and sd["base_lrs"] == sc.BASES
    rest = _run(a, opt, 5)
    opt2 = _opt()
    b = sc.make_scheduler("cosine", opt2, 3, 0.1, 3)
    b.load_state_dict(sd)
    assert b.last_epoch == 7
    assert _run(b, opt2, 5) == rest


@pytest.mark.parametrize("make", [
    lambda L, o: L.WarmupCosineLR(o, 3, warmup_steps=3),
    lambda L, o: L.WarmupPolyLR(o, 2, warmup_steps=5),
    lambda L, o: L.WarmupMultiStepLR(o, [9, 4]),
    lambda L, o: L.WarmupMultiStepLR(o, list(range(1, 10))),
    lambda L, o: L.WarmupConstantLR(o, period=0),
    lambda L, o: L.WarmupConstantLR(o, warmup_steps=-1),
], ids=["total_eq_warmup", "total_lt_warmup", "unsorted", "nine_milestones", "period_0", "negative_warmup"])
def test_argument_validation(make):
    from ringdp.optim import lr_scheduler as L

    with pytest.raises(ValueError):
        make(L, _opt())


def test_exports():
    import ringdp
    from ringdp.optim.lr_scheduler import (DeviceLR, WarmupConstantLR, WarmupCosineLR, WarmupMultiStepLR,  # noqa: F401
                                           WarmupPolyLR)
    from ringdp.utils import ModelEma  # noqa: F401

    assert ringdp.optim.lr_scheduler.DeviceLR is DeviceLR
    assert all(issubclass(c, DeviceLR) for c in (WarmupConstantLR, WarmupCosineLR, WarmupMultiStepLR, WarmupPolyLR))


def test_native_ops_fail_loudly_on_bad_input():
    import ringdp

    C = ringdp._C
    t, n, spec = torch.zeros(()), torch.zeros((), dtype=torch.int64), ringdp._C.LrSchedSpec()
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.lr_sched_run(n, spec, [0.1], [t], True)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.ema_tick_run(n, t, 0.9, False)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.ema_update_flat(torch.zeros(8), torch.zeros(8), t)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        C.adam_table_build([torch.zeros(8)], [torch.zeros(8)], [], [], [1])


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_ema_foreach_lerp(decay, warmup):
    """6 updates with changing parameters against the same recurrence in fp64 with the fp32-rounded weight.
    Bound: all values stay below 8 in magnitude (asserted), where half an fp32 ulp is 2.4e-7.  ATen's lerp rounds at
    most 4 times per element (difference, 1 - w, product, sum) and its 1 - w carries 6e-8 of |p - e| < 10, so one
    update is within 4 * 2.4e-7 + 6e-7 = 1.6e-6 of the exact one; earlier errors are carried with a factor
    1 - w <= 1, so 6 updates stay within 1e-5.  Leaving the update out would miss by w * |p - e| ~ 1e-4 or more."""
    from ringdp.utils import ModelEma

    model = sc.Bag(values(SHAPES))
    ema = ModelEma(model, decay=decay, warmup=warmup)
    assert not ema.module.training and all(not p.requires_grad for p in ema.module.parameters())
    ref = [p.detach().double().clone() for p in model.ps]
    for k in range(6):
        with torch.no_grad():
            for p, v in zip(model.ps, values(SHAPES, seed=20 + k)):
                p.add_(0.1 * v)
                assert float(p.abs().max()) < 8
        ema.update()
        w = sc.ema_weight(k + 1, decay, warmup)
        assert torch.equal(ema._w, w)
        for r, p in zip(ref, model.ps):
            r.add_(w.double() * (p.detach().double() - r))
        for e, r in zip(ema.module.ps, ref):
            torch.testing.assert_close(e.double(), r, rtol=0.0, atol=1e-5)
    assert int(ema.num_updates) == 6 and ema.num_updates.dtype == torch.int64


def test_ema_buffers_state_dict_and_set():
    from ringdp.utils import ModelEma

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    ema = ModelEma(model, decay=0.5)
    with torch.no_grad():
        model[1].running_mean.fill_(2.0)
        model[1].num_batches_tracked.fill_(7)
        model[0].weight.add_(1.0)
    before = ema.module[0].weight.clone()
    ema.update()
    assert torch.equal(ema.module[1].running_mean, torch.full((3,), 1.0))  # the float buffer is averaged
    assert int(ema.module[1].num_batches_tracked) == 7                     # the integer buffer is copied
    torch.testing.assert_close(ema.module[0].weight, before + 0.5, rtol=1e-6, atol=1e-6)
    sd = ema.state_dict()
    assert set(sd) == set(model.state_dict()) | {"num_updates"} and int(sd["num_updates"]) == 1
    other = ModelEma(model, decay=0.5)
    ptrs = [p.data_ptr() for p in other.module.parameters()]
    other.load_state_dict(sd)
    assert ptrs == [p.data_ptr() for p in other.module.parameters()], "the load writes in place"
    assert int(other.num_updates) == 1
    for (ka, a), (kb, b) in zip(other.module.state_dict().items(), ema.module.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    ema.set(model)
    for a, b in zip(ema.module.state_dict().values(), model.state_dict().values()):
        assert torch.equal(a, b)


def test_ema_rejects_bf16_parameters():
    from ringdp.utils import ModelEma

    with pytest.raises(NotImplementedError, match="float32"):
        ModelEma(torch.nn.Linear(4, 3).bfloat16())
