"""AdamW / Adam with fused global-norm gradient clipping.

Math parity: ``torch/optim/adamw.py`` / ``torch/optim/adam.py`` (single-tensor form, amsgrad off) and
``torch.nn.utils.clip_grad_norm_`` for ``max_grad_norm``.

GPU step (kernels in ``csrc/kernels/optim.hip``; G parameter groups):
* ``max_grad_norm`` set: one ``grad_sumsq`` launch over the gradients of every group;
* one ``adam_prepare`` launch: total norm and clip coefficient, step counters += 1, bias corrections, ``lr`` read
  from device memory when it is a tensor - everything that changes between steps stays on the device;
* one update launch per group: flat (a single float4 range) when the parameters were flattened by ringdp's DDP,
  multi-tensor over a cached pointer table otherwise.
So a step is at most ``1 + G`` launches, ``2 + G`` with clipping, with no host sync and, once the table exists, no
allocation: it can be captured by ``ringdp.utils.graph.StepGraph`` and replayed, and a replay advances the step
count and follows ``lr`` changes.  With clipping ``p.grad`` is left untouched (the coefficient is applied inside
the update) and ``opt.grad_norm`` is a 0-dim device tensor holding the last pre-clip norm.

The table is keyed on the addresses of parameters, gradients and moments: gradients written in place (DDP bucket
views, ``zero_grad(set_to_none=False)``, static buffers of a captured step) keep it; gradient tensors at new
addresses rebuild it, with one synchronous upload.  At most 32 parameter groups on the GPU.

State is torch's (``exp_avg``, ``exp_avg_sq``, ``step``), so ``state_dict`` round-trips with ``torch.optim.AdamW``.
``step`` is a 0-dim float32 tensor on the parameter's device, and one counter is shared by the parameters of a
group: a parameter that first receives a gradient later joins its group's count.
CPU: the same math with ATen ops.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.optim.optimizer import Optimizer

from .._native import C
from ..utils import tracing as _tracing
from .sgd import _invalidate_packs

_MAX_GROUPS = 32  # kern::kAdamMaxGroups


def _flat_views(params):
    """(flat_param, flat_grad, offsets) when every param is a view into one DDP-flattened buffer whose grads
    are the matching bucket views (the condition of ``SGD._flat_layout``)."""
    metas = [getattr(p, "_ringdp_flat", None) for p in params]
    if not params or any(m is None for m in metas):
        return None
    fp, fg = metas[0][0], metas[0][1]
    if any(m[0] is not fp or m[1] is not fg for m in metas):
        return None
    if len(params) != metas[0][3]:  # must cover every parameter of the buffer
        return None
    for p, m in zip(params, metas):
        off = m[2]
        if p.grad is None or p.grad.data_ptr() != fg.data_ptr() + off * fg.element_size():
            return None
        if p.data_ptr() != fp.data_ptr() + off * fp.element_size():
            return None
    return fp, fg, [m[2] for m in metas]


class Adam(Optimizer):
    """``torch.optim.Adam`` on ringdp kernels (weight decay added to the gradient)."""

    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, maximize: bool = False, foreach: Optional[bool] = None,
                 capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None,
                 max_grad_norm: Optional[float] = None):
        name = type(self).__name__
        if torch.is_tensor(lr):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
        elif lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise NotImplementedError(f"ringdp.optim.{name}: amsgrad=True is not supported")
        if differentiable:
            raise NotImplementedError(f"ringdp.optim.{name}: differentiable=True is not supported")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm}")
        # torch's group keys, so a state_dict loads into torch.optim.Adam / AdamW and back
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay,
                        amsgrad=False, maximize=maximize, foreach=foreach, capturable=capturable,
                        differentiable=False, fused=fused, decoupled_weight_decay=self._decoupled)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm: Optional[torch.Tensor] = None  # last pre-clip total norm (0-dim, on the params' device)
        self._plan = None  # the GPU step's cached table / record / partials, keyed on addresses
        self._flat_bufs = {}
        self._group_steps = {}

    def state_dict(self):
        sd = super().state_dict()
        # torch's optimizers add 1 to every entry of their step list: hand each parameter a counter of its own,
        # not the group's shared tensor
        def own_step(st):
            st = dict(st)  # the packed state holds the live per-parameter dicts
            if torch.is_tensor(st.get("step")):
                st["step"] = st["step"].clone()
            return st

        sd["state"] = {k: own_step(st) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # drop the fused-kernel layouts: the next step re-adopts the loaded moments
        self._plan = None
        self._flat_bufs = {}
        self._group_steps = {}
        for gi, group in enumerate(self.param_groups):
            have = [p for p in group["params"] if "step" in self.state.get(p, {})]
            if not have:
                continue
            vals = [float(self.state[p]["step"]) for p in have]
            if any(v != vals[0] for v in vals):
                raise ValueError(
                    f"ringdp.optim.{type(self).__name__} keeps one step counter per parameter group, but the "
                    f"loaded state of group {gi} has parameters at different steps {sorted(set(vals))}")
            shared = torch.tensor(vals[0], dtype=torch.float32, device=have[0].device)
            for p in have:
                self.state[p]["step"] = shared
            self._group_steps[gi] = shared

    # ------------------------------------------------------------------ helpers
    def _group_step(self, gi, params):
        step = self._group_steps.get(gi)
        if step is None:
            step = next((self.state[p]["step"] for p in params if "step" in self.state[p]), None)
            if step is None:
                step = torch.zeros((), dtype=torch.float32, device=params[0].device)
            self._group_steps[gi] = step
        return step

    def _init_state(self, gi, params):
        """Per-parameter state of a group (torch's layout); returns (step, exp_avgs, exp_avg_sqs)."""
        step = self._group_step(gi, params)
        ms, vs = [], []
        for p in params:
            st = self.state[p]
            if "exp_avg" not in st:
                st["step"] = step
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            ms.append(st["exp_avg"])
            vs.append(st["exp_avg_sq"])
        return step, ms, vs

    def _flat_layout(self, gi, params):
        """(flat_param, flat_grad, flat_exp_avg, flat_exp_avg_sq) when the group is one DDP-flattened buffer; the
        per-parameter state entries then are views into the flat moment buffers."""
        lay = _flat_views(params)
        if lay is None:
            return None
        fp, fg, offs = lay
        key = (fp.data_ptr(), gi)
        bufs = self._flat_bufs.get(key)
        if bufs is None or bufs[0].numel() != fp.numel():
            bufs = (torch.zeros_like(fp), torch.zeros_like(fp))
            # adopt any existing per-parameter moments (e.g. after load_state_dict)
            for p, off in zip(params, offs):
                st = self.state[p]
                for flat, name in zip(bufs, ("exp_avg", "exp_avg_sq")):
                    if st.get(name) is not None:
                        flat[off:off + p.numel()].copy_(st[name].reshape(-1))
            self._flat_bufs[key] = bufs
        step = self._group_step(gi, params)
        for p, off in zip(params, offs):
            st = self.state[p]
            for flat, name in zip(bufs, ("exp_avg", "exp_avg_sq")):
                cur = st.get(name)
                if cur is None or cur.data_ptr() != flat.data_ptr() + off * flat.element_size():
                    st[name] = flat[off:off + p.numel()].view_as(p)
            if "step" not in st:
                st["step"] = step
        return fp, fg, bufs[0], bufs[1]

    @staticmethod
    def _hyper(group) -> "C.AdamHyper":
        h = C.AdamHyper()
        lr = group["lr"]
        h.lr = 0.0 if (torch.is_tensor(lr) and lr.is_cuda) else float(lr)
        h.beta1, h.beta2 = float(group["betas"][0]), float(group["betas"][1])
        h.eps = float(group["eps"])
        h.weight_decay = float(group["weight_decay"])
        h.maximize = bool(group["maximize"])
        h.decoupled = bool(group.get("decoupled_weight_decay", False))
        return h

    # ------------------------------------------------------------------ step
    @torch.no_grad()
    @_tracing.annotate("ringdp.AdamW.step")
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        gpu, cpu = [], []
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            if group.get("amsgrad", False):
                raise NotImplementedError(f"ringdp.optim.{type(self).__name__}: amsgrad=True is not supported")
            (gpu if params[0].is_cuda else cpu).append((gi, group, params))
        if gpu and cpu and self.max_grad_norm is not None:
            raise NotImplementedError("max_grad_norm over parameter groups on both CPU and GPU is not supported")
        if gpu:
            self._step_gpu(gpu)
        if cpu:
            self._step_cpu(cpu)
        return loss

    def _step_gpu(self, groups):
        if len(groups) > _MAX_GROUPS:
            raise NotImplementedError(f"ringdp.optim.{type(self).__name__}: at most {_MAX_GROUPS} parameter groups "
                                      f"on the GPU, got {len(groups)}")
        clip = self.max_grad_norm is not None
        ps, gs, ms, vs, sizes, flats, steps, key = [], [], [], [], [], [], [], [clip]
        for gi, group, params in groups:
            flat = self._flat_layout(gi, params)
            if flat is not None:
                step = self._group_steps[gi]
                gms = [self.state[p]["exp_avg"] for p in params]
                gvs = [self.state[p]["exp_avg_sq"] for p in params]
                key.append(tuple(t.data_ptr() for t in flat) + (flat[0].numel(),))
            else:
                step, gms, gvs = self._init_state(gi, params)
                key.append(None)
            ggs = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]
            flats.append(flat)
            steps.append(step)
            sizes.append(len(params))
            ps += params
            gs += ggs
            ms += gms
            vs += gvs
            key.append(step.data_ptr())
        key += [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                for p, g, m, v in zip(ps, gs, ms, vs)]
        plan = self._plan
        if plan is None or plan[0] != key:
            # Pointer table cached per addresses: the one synchronous upload happens here, outside any capture;
            # later steps over the same tensors allocate nothing and are hipGraph-capturable.
            table = C.adam_table_build(ps, gs, ms, vs, sizes)
            dev = ps[0].device
            rec = torch.zeros(4 + 4 * len(groups), dtype=torch.float32, device=dev)
            partials = torch.zeros(table.nchunks, dtype=torch.float32, device=dev) if clip else None
            plan = self._plan = (key, table, rec, partials)
            self.grad_norm = rec[0] if clip else None
        _, table, rec, partials = plan
        hypers = [self._hyper(group) for _, group, _ in groups]
        lrs = [group["lr"] if (torch.is_tensor(group["lr"]) and group["lr"].is_cuda) else None
               for _, group, _ in groups]
        if clip:
            C.grad_sumsq_run(table, partials)
        C.adam_prepare_run(rec, partials, table.nchunks if clip else 0, self.max_grad_norm if clip else 0.0,
                           steps, lrs, hypers)
        for k, flat in enumerate(flats):
            if flat is not None:
                C.adam_update_flat(flat[0], flat[1], flat[2], flat[3], rec, k, hypers[k])
            else:
                C.adam_update_run(table, k, rec, k, hypers[k])
        _invalidate_packs(ps)

    def _step_cpu(self, groups):
        coef = None
        if self.max_grad_norm is not None:
            norms = torch._foreach_norm([p.grad for _, _, params in groups for p in params])
            total = torch.linalg.vector_norm(torch.stack(norms))
            coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
            self.grad_norm = total
        for gi, group, params in groups:
            step, ms, vs = self._init_state(gi, params)
            step += 1
            t = float(step)
            lr, wd, eps = float(group["lr"]), group["weight_decay"], group["eps"]
            b1, b2 = group["betas"]
            step_size = lr / (1 - b1 ** t)
            bc2_sqrt = math.sqrt(1 - b2 ** t)
            for p, m, v in zip(params, ms, vs):
                g = p.grad if coef is None else p.grad * coef
                if group["maximize"]:
                    g = -g
                if group.get("decoupled_weight_decay", False):
                    p.mul_(1 - lr * wd)
                elif wd != 0:
                    g = g.add(p, alpha=wd)
                m.lerp_(g, 1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = (v.sqrt() / bc2_sqrt).add_(eps)
                p.addcdiv_(m, denom, value=-step_size)


class AdamW(Adam):
    """``torch.optim.AdamW`` on ringdp kernels (decoupled weight decay)."""

    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False, foreach: Optional[bool] = None,
                 capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None,
                 max_grad_norm: Optional[float] = None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, foreach=foreach,
                         capturable=capturable, differentiable=differentiable, fused=fused,
                         max_grad_norm=max_grad_norm)
