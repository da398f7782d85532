"""Learning-rate schedules evaluated on the device.

``ringdp.optim.SGD`` and ``AdamW`` / ``Adam`` read ``lr`` from a 0-dim fp32 device tensor; the schedulers here
write that tensor from a device-resident step counter, so the schedule advances inside a captured
``ringdp.utils.graph.StepGraph`` step with no host value in the loop.

The factor (this is the contract; kernel ``lr_sched_kernel`` in ``csrc/kernels/sched_ema.hip`` and the CPU path
evaluate the same expressions in fp64).  With ``t`` the number of ``step()`` calls so far::

    s = t // period                      W = warmup_steps          a = warmup_start_factor
    N = total_steps - W   (N >= 1)       m = min_factor            u = min(max(s - W, 0), N)

    s < W :      f = a + (1 - a) * s / W
    otherwise :  constant    f = 1
                 cosine      f = m + (1 - m) * (1 + cos(pi * u / N)) / 2
                 poly        f = m + (1 - m) * (1 - u / N) ** power          (power = 1: linear decay)
                 multistep   f = gamma ** (number of milestones <= s)        (at most 8 milestones)

and ``lr_g(t) = float32(initial_lr_g * f)`` for every parameter group ``g``.  ``warmup_steps``, ``total_steps``
and ``milestones`` count in units of ``s``; ``period`` (``step()`` calls per unit) lets an epoch-wise schedule live
inside a per-iteration captured step.  Past ``total_steps`` the value stays at its end point.

Semantics are torch's: construction records each group's ``lr`` as ``initial_lr`` and sets ``lr(0)``; call
``step()`` after ``optimizer.step()``; after ``k`` calls the groups hold ``lr(k)``.

GPU (parameters on a GPU): ``group["lr"]`` becomes a 0-dim fp32 device tensor (one that is already there is kept
and written in place, so graphs captured earlier stay valid) and ``step()`` is one launch of one workgroup: no
host sync, no allocation, at most 32 parameter groups.  CPU: the same closed form on the host, ``group["lr"]``
stays a Python float.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import torch

from .._native import C

_MAX_GROUPS = 32     # kern::kAdamMaxGroups
_MAX_MILESTONES = 8  # kern::kSchedMaxMilestones
_KINDS = {"constant": 0, "cosine": 1, "poly": 2, "multistep": 3}  # kern::SchedKind


def schedule_factor(t: int, *, kind: str, total_steps: int, warmup_steps: int = 0, warmup_start_factor: float = 0.0,
                    period: int = 1, min_factor: float = 0.0, power: float = 1.0, milestones: Sequence[int] = (),
                    gamma: float = 0.1) -> float:
    """The factor ``f`` of the module docstring at counter value ``t``, in Python floats (fp64)."""
    s = t // period
    W = warmup_steps
    if s < W:
        a = warmup_start_factor
        return a + (1.0 - a) * s / W
    N = total_steps - W
    u = min(max(s - W, 0), N)
    m = min_factor
    if kind == "cosine":
        return m + (1.0 - m) * (1.0 + math.cos(math.pi * u / N)) / 2.0
    if kind == "poly":
        return m + (1.0 - m) * (1.0 - u / N) ** power
    if kind == "multistep":
        return gamma ** sum(1 for ms in milestones if ms <= s)
    return 1.0


class DeviceLR:
    """Base class: warmup, then the factor of ``kind`` (see the module docstring)."""

    def __init__(self, optimizer, *, kind: str = "constant", total_steps=None, warmup_steps: int = 0,
                 warmup_start_factor: float = 0.0, period: int = 1, min_factor: float = 0.0, power: float = 1.0,
                 milestones: Sequence[int] = (), gamma: float = 0.1):
        if kind not in _KINDS:
            raise ValueError(f"unknown schedule kind {kind!r}")
        warmup_steps, period = int(warmup_steps), int(period)
        if total_steps is None:  # constant / multistep have no horizon
            total_steps = warmup_steps + 1
        spec = dict(kind=kind, total_steps=int(total_steps), warmup_steps=warmup_steps,
                    warmup_start_factor=float(warmup_start_factor), period=period, min_factor=float(min_factor),
                    power=float(power), milestones=[int(m) for m in milestones], gamma=float(gamma))
        self._check_spec(spec)
        self.optimizer = optimizer
        self.spec = spec
        groups = optimizer.param_groups
        devs = {p.device for g in groups for p in g["params"]}
        if not devs:
            raise ValueError("DeviceLR: the optimizer has no parameters")
        if len(devs) > 1:
            raise NotImplementedError(f"DeviceLR: parameters on several devices {sorted(map(str, devs))}")
        self.device = next(iter(devs))
        self._gpu = self.device.type == "cuda"
        if self._gpu and len(groups) > _MAX_GROUPS:
            raise NotImplementedError(f"DeviceLR: at most {_MAX_GROUPS} parameter groups on the GPU, "
                                      f"got {len(groups)}")
        for g in groups:
            if "initial_lr" not in g:
                g["initial_lr"] = float(g["lr"])
        self._t = 0
        self._cspec = None
        if self._gpu:
            self._counter = torch.zeros((), dtype=torch.int64, device=self.device)
        self._evaluate(advance=False)

    # ------------------------------------------------------------------ checks
    @staticmethod
    def _check_spec(spec):
        if spec["period"] < 1:
            raise ValueError(f"period must be at least 1, got {spec['period']}")
        if spec["warmup_steps"] < 0:
            raise ValueError(f"warmup_steps must not be negative, got {spec['warmup_steps']}")
        if spec["total_steps"] <= spec["warmup_steps"]:
            raise ValueError(f"total_steps ({spec['total_steps']}) must exceed warmup_steps "
                             f"({spec['warmup_steps']})")
        ms = spec["milestones"]
        if len(ms) > _MAX_MILESTONES:
            raise ValueError(f"at most {_MAX_MILESTONES} milestones, got {len(ms)}")
        if any(a > b for a, b in zip(ms, ms[1:])):
            raise ValueError(f"milestones must be sorted, got {ms}")

    def _lr_tensors(self) -> List[torch.Tensor]:
        """The groups' device lr tensors, installed where a group still holds a number."""
        out = []
        for gi, g in enumerate(self.optimizer.param_groups):
            lr = g["lr"]
            if not torch.is_tensor(lr):
                lr = g["lr"] = torch.full((), float(lr), dtype=torch.float32, device=self.device)
            elif lr.dim() != 0 or lr.dtype != torch.float32 or lr.device != self.device:
                raise ValueError(f"DeviceLR: the lr tensor of group {gi} must be a 0-dim float32 tensor on "
                                 f"{self.device}, got shape {tuple(lr.shape)} {lr.dtype} on {lr.device}")
            out.append(lr)
        return out

    # ------------------------------------------------------------------ evaluation
    def _native_spec(self):
        if self._cspec is None:
            s = C.LrSchedSpec()
            s.kind = _KINDS[self.spec["kind"]]
            for k in ("period", "warmup_steps", "total_steps", "warmup_start_factor", "min_factor", "power", "gamma",
                      "milestones"):
                setattr(s, k, self.spec[k])
            self._cspec = s
        return self._cspec

    def _evaluate(self, advance: bool):
        groups = self.optimizer.param_groups
        if not self._gpu:
            if advance:
                self._t += 1
            f = schedule_factor(self._t, **self.spec)
            for g in groups:
                g["lr"] = g["initial_lr"] * f
            return
        if len(groups) > _MAX_GROUPS:
            raise NotImplementedError(f"DeviceLR: at most {_MAX_GROUPS} parameter groups on the GPU, "
                                      f"got {len(groups)}")
        lrs, bases, seen = [], [], {}
        for g, lr in zip(groups, self._lr_tensors()):
            base = float(g["initial_lr"])
            prev = seen.get(lr.data_ptr())
            if prev is None:  # groups created from one tensor default share it: written once
                seen[lr.data_ptr()] = base
                lrs.append(lr)
                bases.append(base)
            elif prev != base:
                raise ValueError("DeviceLR: parameter groups that share one lr tensor must share initial_lr, got "
                                 f"{prev} and {base}")
        C.lr_sched_run(self._counter, self._native_spec(), bases, lrs, advance)

    def step(self):
        """Advance the counter by one and write every group's lr (GPU: one launch, capturable)."""
        self._evaluate(advance=True)

    # ------------------------------------------------------------------ host API
    @property
    def last_epoch(self) -> int:
        """The number of ``step()`` calls so far (synchronises on the GPU)."""
        return int(self._counter.item()) if self._gpu else self._t

    @property
    def base_lrs(self) -> List[float]:
        return [float(g["initial_lr"]) for g in self.optimizer.param_groups]

    def get_last_lr(self) -> List[float]:
        """The current lr of every group as floats (synchronises on the GPU)."""
        return [float(g["lr"]) for g in self.optimizer.param_groups]

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "spec": dict(self.spec, milestones=list(self.spec["milestones"])),
                "base_lrs": self.base_lrs}

    def load_state_dict(self, state):
        spec = dict(state["spec"])
        spec["milestones"] = [int(m) for m in spec["milestones"]]
        if spec["kind"] not in _KINDS:
            raise ValueError(f"unknown schedule kind {spec['kind']!r}")
        self._check_spec(spec)
        bases = state["base_lrs"]
        if len(bases) != len(self.optimizer.param_groups):
            raise ValueError(f"loaded state has {len(bases)} parameter groups, the optimizer has "
                             f"{len(self.optimizer.param_groups)}")
        self.spec, self._cspec = spec, None
        for g, b in zip(self.optimizer.param_groups, bases):
            g["initial_lr"] = float(b)
        n = int(state["last_epoch"])
        if self._gpu:
            self._counter.fill_(n)  # in place: a captured step keeps reading this address
        else:
            self._t = n
        self._evaluate(advance=False)


class WarmupCosineLR(DeviceLR):
    """Linear warmup, then half a cosine from 1 down to ``min_factor`` at ``total_steps``."""

    def __init__(self, optimizer, total_steps: int, min_factor: float = 0.0, *, warmup_steps: int = 0,
                 warmup_start_factor: float = 0.0, period: int = 1):
        super().__init__(optimizer, kind="cosine", total_steps=total_steps, min_factor=min_factor,
                         warmup_steps=warmup_steps, warmup_start_factor=warmup_start_factor, period=period)


class WarmupPolyLR(DeviceLR):
    """Linear warmup, then ``(1 - u / N) ** power`` from 1 down to ``min_factor`` (``power=1``: linear decay)."""

    def __init__(self, optimizer, total_steps: int, power: float = 1.0, min_factor: float = 0.0, *,
                 warmup_steps: int = 0, warmup_start_factor: float = 0.0, period: int = 1):
        super().__init__(optimizer, kind="poly", total_steps=total_steps, power=power, min_factor=min_factor,
                         warmup_steps=warmup_steps, warmup_start_factor=warmup_start_factor, period=period)


class WarmupMultiStepLR(DeviceLR):
    """Linear warmup, then ``gamma`` to the number of milestones passed (at most 8, sorted)."""

    def __init__(self, optimizer, milestones: Sequence[int], gamma: float = 0.1, *, warmup_steps: int = 0,
                 warmup_start_factor: float = 0.0, period: int = 1):
        super().__init__(optimizer, kind="multistep", milestones=milestones, gamma=gamma,
                         warmup_steps=warmup_steps, warmup_start_factor=warmup_start_factor, period=period)


class WarmupConstantLR(DeviceLR):
    """Linear warmup, then the base lr."""

    def __init__(self, optimizer, *, warmup_steps: int = 0, warmup_start_factor: float = 0.0, period: int = 1):
        super().__init__(optimizer, kind="constant", warmup_steps=warmup_steps,
                         warmup_start_factor=warmup_start_factor, period=period)
