"""Shared pieces of the LR-schedule and model-EMA tests: the fp64 closed forms written out, the cases, the torch
scheduler references, the EMA element contract on the CPU, and an ulp distance for fp32 tensors.

Gates.  Schedules: ringdp and the closed form below both evaluate the factor in fp64 and round ``base_lr * f`` to
fp32 once, so they may differ by the last fp64 bits of ``cos`` / ``pow`` only: at most 1 fp32 ulp.  torch's
schedulers use recursive fp64 forms; they agree with the closed form far below fp32 rounding (6e-8): rtol 1e-6.
EMA: the contract is ``d = p - e; e = fma(w, d, e)`` in fp32; the CPU reference emulates the fma in fp64
(``w * d`` is exact there, the sum is rounded to fp64 and then to fp32), so double rounding is the only
difference: at most 1 ulp."""
import functools
import math

import torch

# short horizons: warmup 3, the end at 17, milestones inside the horizon
TOTAL, MILESTONES, GAMMA = 17, [4, 9], 0.1
BASES = [0.05, 0.003]  # two groups with different base lrs
# (warmup_steps, warmup_start_factor): a warmup, no warmup, a warmup from zero
WARMUPS = [(3, 0.1), (0, 0.0), (3, 0.0)]
PERIODS = [1, 3]
# name -> (class name, constructor kwargs, kind, the closed form's parameters)
KINDS = {
    "cosine": ("WarmupCosineLR", dict(total_steps=TOTAL, min_factor=0.05)),
    "poly_linear": ("WarmupPolyLR", dict(total_steps=TOTAL, power=1.0, min_factor=0.0)),
    "poly_2": ("WarmupPolyLR", dict(total_steps=TOTAL, power=2.0, min_factor=0.1)),
    "multistep": ("WarmupMultiStepLR", dict(milestones=MILESTONES, gamma=GAMMA)),
    "constant": ("WarmupConstantLR", dict()),
}


def closed_form(name, t, W, a, period):
    """The issue's factor definition, in Python floats (fp64)."""
    kw = KINDS[name][1]
    s = t // period
    if s < W:
        return a + (1 - a) * s / W
    if name == "constant":
        return 1.0
    if name == "multistep":
        return kw["gamma"] ** sum(1 for ms in kw["milestones"] if ms <= s)
    N = kw["total_steps"] - W
    u = min(max(s - W, 0), N)
    m = kw["min_factor"]
    if name == "cosine":
        return m + (1 - m) * (1 + math.cos(math.pi * u / N)) / 2
    return m + (1 - m) * (1 - u / N) ** kw["power"]


def steps_for(period):
    """k = 0 .. total_steps + 5 in schedule units, i.e. that many periods of step() calls."""
    return (TOTAL + 5) * period + 1


def expected_lrs(name, W, a, period, bases=BASES):
    """fp32 tensor [steps, groups]: float32(base * f(k)) from the closed form."""
    rows = [[b * closed_form(name, k, W, a, period) for b in bases] for k in range(steps_for(period))]
    return torch.tensor(rows, dtype=torch.float64).float()


def make_scheduler(name, opt, W, a, period):
    from ringdp.optim import lr_scheduler

    cls, kw = KINDS[name]
    return getattr(lr_scheduler, cls)(opt, warmup_steps=W, warmup_start_factor=a, period=period, **kw)


def ordered_int(x):
    """fp32 tensor -> int64 whose differences count representable values between two floats."""
    i = x.contiguous().view(torch.int32).long()
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


def ulp_report(got, want):
    """(largest ulp distance, number of unequal elements) between two fp32 CPU tensors."""
    d = (ordered_int(got.reshape(-1)) - ordered_int(want.reshape(-1))).abs()
    return int(d.max()) if d.numel() else 0, int((d != 0).sum())


@functools.lru_cache(maxsize=None)
def torch_reference(name):
    """lr(k), k = 0 .. TOTAL + 5, of the matching torch scheduler on fp64 CPU parameters, W = 0 (for 'linear_warmup':
    LinearLR over 3 steps from 0.1).  fp64 tensor [steps, groups]."""
    ps = [torch.zeros(2, dtype=torch.float64, requires_grad=True) for _ in BASES]
    opt = torch.optim.SGD([dict(params=[p], lr=b) for p, b in zip(ps, BASES)])
    S = torch.optim.lr_scheduler
    if name == "cosine":
        sch = S.CosineAnnealingLR(opt, T_max=TOTAL, eta_min=0.0)
    elif name == "poly_linear":
        sch = S.PolynomialLR(opt, total_iters=TOTAL, power=1.0)
    elif name == "poly_2":
        sch = S.PolynomialLR(opt, total_iters=TOTAL, power=2.0)
    elif name == "multistep":
        sch = S.MultiStepLR(opt, milestones=MILESTONES, gamma=GAMMA)
    else:
        sch = S.LinearLR(opt, start_factor=0.1, end_factor=1.0, total_iters=3)
    rows = []
    for _ in range(TOTAL + 6):
        rows.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sch.step()
    return torch.tensor(rows, dtype=torch.float64)


def ringdp_for_torch(name, opt):
    """The ringdp scheduler that the torch scheduler of ``torch_reference(name)`` corresponds to."""
    from ringdp.optim import lr_scheduler as L

    if name == "cosine":
        return L.WarmupCosineLR(opt, TOTAL, 0.0)
    if name == "poly_linear":
        return L.WarmupPolyLR(opt, TOTAL, 1.0)
    if name == "poly_2":
        return L.WarmupPolyLR(opt, TOTAL, 2.0)
    if name == "multistep":
        return L.WarmupMultiStepLR(opt, MILESTONES, GAMMA)
    return L.WarmupConstantLR(opt, warmup_steps=3, warmup_start_factor=0.1)


TORCH_NAMES = ["cosine", "poly_linear", "poly_2", "multistep", "linear_warmup"]


def torch_rows(name):
    """Rows of the torch reference that are comparable: CosineAnnealingLR is periodic past T_max, where the
    contract holds the end point instead."""
    return TOTAL + 1 if name == "cosine" else TOTAL + 6


# ---------------------------------------------------------------------------------------------- EMA
def ema_weight(n, decay, warmup):
    """float32(1 - decay_n) after the n-th update, from the fp64 formula."""
    d = min(decay, (1 + n) / (10 + n)) if warmup else decay
    return torch.tensor(1 - d, dtype=torch.float64).float()


def ema_contract(e, p, w):
    """One update of the contract on fp32 CPU tensors: d = p - e in fp32, then the fma emulated in fp64."""
    d = p - e
    assert d.dtype == torch.float32
    return (w.double() * d.double() + e.double()).float()


class Bag(torch.nn.Module):
    """A module over given leaf tensors: the parameters share their storage (and so their alignment)."""

    def __init__(self, leaves):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.detach()) for t in leaves])
        for p, t in zip(self.ps, leaves):
            assert p.data_ptr() == t.data_ptr()
