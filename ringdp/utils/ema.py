"""Exponential moving average of a model's weights (timm's ``ModelEmaV2``), hipGraph-safe.

``ema = ModelEma(model, decay=0.9999, warmup=False)`` deep-copies the module (a ringdp ``DistributedDataParallel``
is unwrapped) into ``ema.module``, in ``eval()`` mode with ``requires_grad_(False)``; ``ema.update()`` after each
optimizer step moves the copy towards the live weights.

Element definition (the contract), in fp32, for every fp32 parameter and floating-point buffer::

    n = num_updates + 1                                    (int64, on the parameters' device)
    decay_n = decay                                        or, with warmup=True, min(decay, (1 + n) / (10 + n))
    w = float32(1 - decay_n)                               (fp64, rounded once)
    d = p - e;  e = fma(w, d, e)

Integer buffers (``num_batches_tracked``) are copied.  Parameters that are not fp32 raise.

GPU (kernels in ``csrc/kernels/sched_ema.hip``): ``ema_tick`` (one thread: ``n`` and ``w`` stay on the device, so a
captured step replays with the right warmup decay), then ``ema_update`` - flat, one float4 range per buffer, when
the source parameters are views of a DDP-flattened buffer (the shadow then owns a matching flat buffer and
``ema.module``'s parameters are views into it), multi-tensor over a cached pointer table for everything else.  The
table is keyed on addresses and rebuilt only when they change: that rebuild is the one synchronous upload and must
happen outside a capture (run ``update()`` once in the warm-up steps, as ``StepGraph`` does).  No atomics; every
element is written by one thread, so updates are bitwise reproducible and flat and multi-tensor forms agree bitwise.
CPU: ``torch._foreach_lerp_`` with the same ``w``.

Precision: the shadow is fp32.  At ``w = 1e-4`` an update smaller than half an ulp of ``e`` (|p - e| below about
6e-4 |e|) is rounded away, exactly as in timm's fp32 ``lerp_``; there is no fp64 or compensated shadow.
"""
from __future__ import annotations

import copy

import torch

from .._native import C


def _unwrap(model):
    from ..parallel import DistributedDataParallel

    return model.module if isinstance(model, DistributedDataParallel) else model


def _own_pack_states(module) -> None:
    """A deep copy carries a copy of the source ConvNet's packed-fragment cache: give the shadow a fresh one of its
    own, registered like any other (``StepGraph.replay`` walks the registry)."""
    from ..ops import convnet

    for m in module.modules():
        if "_ringdp_pack_state" in m.__dict__:
            st = convnet.PackState()
            m.__dict__["_ringdp_pack_state"] = st
            convnet._PACK_STATES.add(st)


class ModelEma:
    def __init__(self, model, decay: float = 0.9999, warmup: bool = False):
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"Invalid decay value: {decay}")
        src = _unwrap(model)
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.module = copy.deepcopy(src)
        self.module.eval()
        self.module.requires_grad_(False)
        _own_pack_states(self.module)
        self._source = src
        # matched once: DDP flattening swaps .data, never the Parameter objects; raises on non-fp32 parameters
        self._es, self._ps, self._ints = self._pairs(src)
        first = next(iter(self.module.parameters()), None)
        self.device = first.device if first is not None else torch.device("cpu")
        self.num_updates = torch.zeros((), dtype=torch.int64, device=self.device)
        self._w = torch.zeros((), dtype=torch.float32, device=self.device)  # 1 - decay_n of the last update
        self._plan = None        # (key, [(shadow flat, source flat)], table or None)
        self._flat_shadows = {}  # source flat buffer address -> the shadow's flat buffer

    # ------------------------------------------------------------------ pairing
    def _pairs(self, src):
        """(float shadows, float sources, [(integer shadow, integer source)]) matched by name."""
        es, ps, ints = [], [], []
        sp, sb = dict(src.named_parameters()), dict(src.named_buffers())
        for name, e in self.module.named_parameters():
            p = sp[name]
            if p.dtype != torch.float32:
                raise NotImplementedError(f"ModelEma: parameter {name!r} is {p.dtype}; only float32 parameters are "
                                          f"averaged")
            es.append(e)
            ps.append(p)
        for name, e in self.module.named_buffers():
            b = sb[name]
            if b.dtype == torch.float32:
                es.append(e)
                ps.append(b)
            elif b.dtype.is_floating_point:
                raise NotImplementedError(f"ModelEma: buffer {name!r} is {b.dtype}; only float32 floating-point "
                                          f"buffers are averaged")
            else:
                ints.append((e, b))
        return es, ps, ints

    def _gpu_plan(self, es, ps):
        key = tuple((e.data_ptr(), p.data_ptr(), p.numel(), id(getattr(p, "_ringdp_flat", (None,))[0]))
                    for e, p in zip(es, ps))
        if self._plan is not None and self._plan[0] == key:
            return self._plan
        # sources that are views of one DDP-flattened buffer, covering it
        by_flat = {}
        for e, p in zip(es, ps):
            meta = getattr(p, "_ringdp_flat", None)
            if meta is not None:
                by_flat.setdefault(id(meta[0]), []).append((e, p, meta))
        flats, in_flat = [], set()
        for members in by_flat.values():
            fp = members[0][2][0]
            ok = (len(members) == members[0][2][3] and fp.dtype == torch.float32 and fp.is_contiguous()
                  and fp.data_ptr() % 16 == 0
                  and all(p.data_ptr() == fp.data_ptr() + m[2] * fp.element_size() for _, p, m in members))
            if not ok:
                continue
            sf = self._flat_shadows.get(fp.data_ptr())
            if sf is None or sf.numel() != fp.numel():
                sf = self._flat_shadows[fp.data_ptr()] = torch.zeros_like(fp)
            for e, p, m in members:
                view = sf[m[2]:m[2] + p.numel()].view_as(e)
                if e.data_ptr() != view.data_ptr():
                    view.copy_(e.data)
                    e.data = view
                in_flat.add(id(e))
            flats.append((sf, fp))
        rest = [(e, p) for e, p in zip(es, ps) if id(e) not in in_flat]
        table = None
        if rest:
            # the one synchronous upload; later updates over the same tensors allocate nothing
            table = C.adam_table_build([e for e, _ in rest], [p.detach() for _, p in rest], [], [], [len(rest)])
        # the shadows may have moved into a flat buffer: key on their final addresses
        key = tuple((e.data_ptr(), p.data_ptr(), p.numel(), id(getattr(p, "_ringdp_flat", (None,))[0]))
                    for e, p in zip(es, ps))
        live = {fp.data_ptr() for _, fp in flats}
        self._flat_shadows = {a: sf for a, sf in self._flat_shadows.items() if a in live}
        self._plan = (key, flats, table)
        return self._plan

    # ------------------------------------------------------------------ update
    def _host_weight(self, n: int) -> float:
        d = min(self.decay, (1.0 + n) / (10.0 + n)) if self.warmup else self.decay
        return float(torch.tensor(1.0 - d, dtype=torch.float64).float())

    @torch.no_grad()
    def update(self):
        """One EMA step from the model given at construction (GPU: capturable once the table exists)."""
        es, ps, ints = self._es, self._ps, self._ints
        if self.device.type != "cuda":
            self.num_updates += 1
            w = self._host_weight(int(self.num_updates))
            self._w.fill_(w)
            if es:
                torch._foreach_lerp_(es, [p.detach() for p in ps], w)
        else:
            _, flats, table = self._gpu_plan(es, ps)
            C.ema_tick_run(self.num_updates, self._w, self.decay, self.warmup)
            for sf, fp in flats:
                C.ema_update_flat(sf, fp, self._w)
            if table is not None:
                C.ema_update_run(table, self._w)
        for e, b in ints:
            e.copy_(b)
        self._written()

    def _written(self):
        """The kernels wrote the shadow's weights without bumping versions: its packed fragments are stale."""
        from ..ops.convnet import invalidate_pack

        invalidate_pack(self.module)

    @torch.no_grad()
    def set(self, model=None):
        """Copy the weights and buffers of ``model`` (default: the model given at construction) over the shadow."""
        src = self._source if model is None else _unwrap(model)
        sp, sb = dict(src.named_parameters()), dict(src.named_buffers())
        for name, e in self.module.named_parameters():
            e.copy_(sp[name])
        for name, e in self.module.named_buffers():
            e.copy_(sb[name])
        self._written()

    # ------------------------------------------------------------------ checkpointing
    def state_dict(self):
        sd = self.module.state_dict()
        sd["num_updates"] = self.num_updates.clone()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        n = sd.pop("num_updates")
        self.module.load_state_dict(sd)  # copies in place: the table's addresses stay
        self.num_updates.fill_(int(n))
        self._written()
