"""Dropout and stochastic depth (drop-path) on ringdp's kernels (``csrc/kernels/dropout.hip``).

Mask definition (what the kernels compute, bit for bit; ``tests/dropout_common.py`` reproduces it in numpy):

* generator  Philox4x32-10, key = ``(seed_lo32, seed_hi32)``, counter = ``(g, step_lo32, step_hi32, site)``;
  ``(seed, step)`` come from the forward's snapshot (``ringdp.random.Draw``), ``site`` numbers the dropout sites of
  that forward in call order.
* element mode  ``g`` = index of the group of 8 consecutive elements (flat, row-major): one call serves one
  16-byte bf16 vector, element ``j`` takes the 16-bit half ``(word[j >> 1] >> (16 * (j & 1))) & 0xffff``.
* row mode (stochastic depth)  ``g`` = sample index ``b``, the decision is ``word[0] & 0xffff`` and covers the rows
  ``[b*T, (b+1)*T)``.
* ``thr = clamp(round(p * 65536), 0, 65535)``; keep iff ``u16 >= thr``; ``scale = 65536 / (65536 - thr)`` (fp32):
  the exact inverse of the realised keep probability, so the expectation is unbiased.  ``thr == 0`` is the
  identity and launches nothing.

No mask is stored: the backward regenerates it (``dx = dropout(dy)`` with the same snapshot and site).
"""
from __future__ import annotations

import struct
from typing import Optional, Tuple

import torch

from .._native import C
from ..random import Draw


def quantize_p(p: float) -> Tuple[int, float]:
    """``(thr, scale)`` of a drop probability: 16-bit threshold and the fp32 scale of the kept elements."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    thr = min(max(int(round(p * 65536.0)), 0), 65535)
    scale = struct.unpack("f", struct.pack("f", 65536.0 / (65536 - thr)))[0]
    return thr, scale


def drop_path_schedule(p: float, num_layers: int):
    """Per-layer stochastic-depth probabilities: linear from 0 (first layer) to ``p`` (last), as DeiT."""
    if num_layers <= 1:
        return [0.0] * max(num_layers, 0)
    return [float(p) * l / (num_layers - 1) for l in range(num_layers)]


def _bf16_rows(t: torch.Tensor, what: str) -> None:
    if t.dtype != torch.bfloat16:
        raise TypeError(f"ringdp.ops.dropout.{what}: the GPU kernels take bf16, got {t.dtype} "
                        "(there is no ATen fallback on the GPU)")


class DropoutF(torch.autograd.Function):
    """``y = m * x`` with ``m = m_row * m_elem`` of ``(snapshot, site, thr)`` / ``(snapshot, site_r, thr_r, T)``."""

    @staticmethod
    def forward(ctx, x, snapshot, site: int, thr: int, site_r: int = 0, thr_r: int = 0, T: int = 0):
        ctx.snapshot = snapshot
        ctx.cfg = (site, thr, site_r, thr_r, T)
        return C.dropout_bf16(x, snapshot, site, thr, site_r, thr_r, T)

    @staticmethod
    def backward(ctx, dy):
        dx = C.dropout_bf16(dy.contiguous(), ctx.snapshot, *ctx.cfg)
        return dx, None, None, None, None, None, None


class DropoutAddF(torch.autograd.Function):
    """``y = res + m_row * m_elem * x`` rounded to bf16 once.  Backward: ``(m * dy, dy)`` - ``dy`` itself is handed
    on as the residual's gradient, so ``LayerNormFork.backward`` still receives it as ``dres``."""

    @staticmethod
    def forward(ctx, x, res, snapshot, site_e: int, thr_e: int, site_r: int = 0, thr_r: int = 0, T: int = 0):
        ctx.snapshot = snapshot
        ctx.cfg = (site_e, thr_e, site_r, thr_r, T)
        return C.dropout_add_bf16(x, res, snapshot, site_e, thr_e, site_r, thr_r, T)

    @staticmethod
    def backward(ctx, dy):
        dx = None
        if ctx.needs_input_grad[0]:
            dx = C.dropout_bf16(dy.contiguous(), ctx.snapshot, *ctx.cfg)
        dres = dy if ctx.needs_input_grad[1] else None
        return dx, dres, None, None, None, None, None, None


def dropout(x: torch.Tensor, p: float, training: bool = True, draw: Optional[Draw] = None) -> torch.Tensor:
    """Element dropout.  GPU bf16 tensors run ringdp's kernel (a stand-alone call makes its own draw: one tick
    launch); CPU tensors go to ATen; anything else on the GPU raises.  On the GPU the threshold is clamped to 65535:
    ``p = 1`` keeps 1 element in 65536 (scaled by 65536), where ATen returns zeros."""
    thr, _ = quantize_p(p)
    if not training or thr == 0:
        return x
    if not x.is_cuda:
        return torch.nn.functional.dropout(x, p, True)
    _bf16_rows(x, "dropout")
    draw = draw if draw is not None else Draw(x.device)
    return DropoutF.apply(x, draw.snapshot, draw.site(), thr)


def dropout_add(x: torch.Tensor, res: torch.Tensor, p: float, training: bool = True, draw: Optional[Draw] = None,
                drop_path: float = 0.0, T: int = 0) -> torch.Tensor:
    """``res + drop_path(dropout(x))`` in one pass over bf16 GPU rows ``[B*T, D]``; ``drop_path`` drops whole
    samples of ``T`` rows.  Sites are taken from ``draw`` in the order (element, row), each only when it is on."""
    thr_e, _ = quantize_p(p if training else 0.0)
    thr_r, _ = quantize_p(drop_path if training else 0.0)
    if not x.is_cuda:
        h = torch.nn.functional.dropout(x, p, training)
        return res + drop_path_rows(h, drop_path, training, T)
    _bf16_rows(x, "dropout_add")
    _bf16_rows(res, "dropout_add")
    if thr_e or thr_r:
        draw = draw if draw is not None else Draw(x.device)
    snapshot = draw.snapshot if draw is not None else None
    site_e = draw.site() if thr_e else 0
    site_r = draw.site() if thr_r else 0
    return DropoutAddF.apply(x, res, snapshot, site_e, thr_e, site_r, thr_r, T if thr_r else 0)


def drop_path_rows(x: torch.Tensor, p: float, training: bool, T: int = 0) -> torch.Tensor:
    """ATen stochastic depth: ``x`` is ``[B, ...]`` or, with ``T``, rows ``[B*T, D]``; whole samples are zeroed with
    probability ``p`` and the others scaled by ``1 / (1 - p)``."""
    if not training or p <= 0.0:
        return x
    B = x.shape[0] // T if T else x.shape[0]
    keep = (torch.rand(B, device=x.device) >= p).to(x.dtype) / max(1.0 - p, 2.0 ** -16)
    if T:
        return (x.view(B, T, -1) * keep.view(B, 1, 1)).view_as(x)
    return x * keep.view([B] + [1] * (x.dim() - 1))
