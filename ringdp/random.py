"""ringdp.random - the device-resident generator state behind dropout and stochastic depth.

One small int64 tensor per device holds ``(seed, step)`` (read as unsigned 64-bit values by the kernels).  Its
address never changes, so a captured hipGraph step (``ringdp.utils.graph.StepGraph``) keeps advancing it: a
forward that draws masks starts with one ``rng_tick`` launch (``Draw``), which sets ``step += 1`` on the device and
writes ``(seed, step)`` into a fresh snapshot tensor.  Every dropout site of that forward and of its backward reads
the snapshot, never the live state, so forward, forward, backward, backward uses the right masks, and under capture
the snapshot is a graph-pool buffer that each replay rewrites.  The same design as the Adam step counter
(``adam_prepare``): nothing that changes from step to step lives on the host.

A mask depends on ``(seed, step, site, position)`` only (Philox4x32-10, see ``ringdp.ops.dropout``), so
``manual_seed`` / ``set_rng_state`` make a run reproducible, and the ``(seed, step)`` tuple of plain ints can
travel in a checkpoint's meta (``checkpoint.save(..., rng=ringdp.random.get_rng_state())``).

Default seed at first use: ``torch.initial_seed()`` plus the rank when the process group is initialised -
identical masks on every rank would correlate the replicas' noise in DDP.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

_MASK64 = (1 << 64) - 1
_STATES: Dict[int, torch.Tensor] = {}


def default_seed(initial_seed: int, rank: int) -> int:
    """The seed a device's state starts from: ``initial_seed + rank`` (mod 2^64)."""
    return (int(initial_seed) + int(rank)) & _MASK64


def _signed(v: int) -> int:
    v &= _MASK64
    return v - (1 << 64) if v >= (1 << 63) else v


def _index(device) -> int:
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, int):
        return device
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError(f"ringdp.random: the generator state lives on a GPU, got device {d}")
    return torch.cuda.current_device() if d.index is None else d.index


def _write(idx: int, seed: int, step: int) -> torch.Tensor:
    host = torch.tensor([_signed(seed), _signed(step)], dtype=torch.int64)
    st = _STATES.get(idx)
    if st is None:
        st = _STATES[idx] = host.to(torch.device("cuda", idx))
    else:
        st.copy_(host)  # in place: captured graphs hold this address
    return st


def state_tensor(device=None) -> torch.Tensor:
    """The live ``(seed, step)`` tensor of ``device`` (created with the default seed at first use)."""
    idx = _index(device)
    st = _STATES.get(idx)
    if st is None:
        from . import distributed as dist

        rank = dist.get_rank() if dist.is_initialized() else 0
        st = _write(idx, default_seed(torch.initial_seed(), rank), 0)
    return st


def manual_seed(seed: int, device=None) -> None:
    """Set the seed of ``device``'s state and its step to 0 (in place)."""
    _write(_index(device), int(seed), 0)


def get_rng_state(device=None) -> Tuple[int, int]:
    """``(seed, step)`` as plain ints; ``step`` counts the ticks since the seed was set."""
    seed, step = state_tensor(device).tolist()
    return seed & _MASK64, step & _MASK64


def set_rng_state(state, device=None) -> None:
    seed, step = state
    _write(_index(device), int(seed), int(step))


class Draw:
    """The masks of one forward (and its backward): ticks the device state once and hands out consecutive site
    ids (0, 1, 2, ...) in call order.  Two sites, or two draws, give independent masks."""

    __slots__ = ("snapshot", "_next")

    def __init__(self, device=None):
        from ._native import C

        self.snapshot = C.rng_tick(state_tensor(device))
        self._next = 0

    def site(self) -> int:
        s = self._next
        self._next += 1
        return s


__all__ = ["default_seed", "manual_seed", "get_rng_state", "set_rng_state", "state_tensor", "Draw"]
