"""ringdp.data.Mixup - Mixup / CutMix of a batch with its flipped self, as timm's ``Mixup`` ("batch" and "elem" modes,
``correct_lam=True``), returning the mixed images and a ``MixedTarget`` for ``ringdp.nn.CrossEntropyLoss``.

On the GPU a call is three launches on ringdp's kernels - ``rng_tick`` (one ``ringdp.random.Draw``: the state's
step advances by exactly one), ``mix_draw`` and ``mix_images`` - and ``lam``, the kind and the box stay in device
memory, so a captured step (``StepGraph``) mixes differently on every replay.  On the CPU the same pairing and box
rule run on torch ops with torch's global generator.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
import torch.nn as nn

from ..ops.mixup import MixedTarget, lam_of, mix_batch

_ONES: Dict[torch.device, torch.Tensor] = {}


def _one(device: torch.device) -> torch.Tensor:
    """A cached ``[1.0]`` per device: the identity path launches nothing."""
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones(1, dtype=torch.float32, device=device)
    return t


def cpu_records(R: int, H: int, W: int, mixup_alpha: float, cutmix_alpha: float, prob: float,
                switch_prob: float) -> torch.Tensor:
    """The records ``mix_draw`` writes (``ringdp.ops.mixup``), drawn on the host with torch's global generator: the
    same decision and box rules, another random stream."""
    rec = torch.zeros(R, 8, dtype=torch.int32)
    lam_view = rec.view(torch.float32)
    lam_view[:, 0] = 1.0
    lam_view[:, 6] = 1.0
    u = torch.rand(R, 2)
    for r in range(R):
        if not (mixup_alpha > 0 or cutmix_alpha > 0) or not float(u[r, 0]) < prob:
            continue
        cut = cutmix_alpha > 0 and (not mixup_alpha > 0 or float(u[r, 1]) < switch_prob)
        alpha = cutmix_alpha if cut else mixup_alpha
        lam0 = float(torch.distributions.Beta(float(alpha), float(alpha)).sample())
        lam_view[r, 6] = lam0
        if not cut:
            rec[r, 1] = 1
            lam_view[r, 0] = lam0
            continue
        ratio = math.sqrt(max(1.0 - lam0, 0.0))
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy = int(torch.randint(H, (1,)))
        cx = int(torch.randint(W, (1,)))
        y0, y1 = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
        x0, x1 = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
        rec[r, 1] = 2
        rec[r, 2:6] = torch.tensor([y0, y1, x0, x1], dtype=torch.int32)
        area = torch.tensor(float((y1 - y0) * (x1 - x0)), dtype=torch.float32)
        lam_view[r, 0] = 1.0 - area / torch.tensor(float(H * W), dtype=torch.float32)  # in fp32, as the kernel
    return rec


def mix_reference(x: torch.Tensor, rec: torch.Tensor) -> torch.Tensor:
    """``mix_images`` on torch ops (any device): the CPU path.  The arithmetic of kind 1 runs in fp32."""
    B, _, H, W = x.shape
    rec = rec.expand(B, 8) if rec.shape[0] == 1 else rec
    lam = rec.contiguous().view(torch.float32)[:, 0].view(B, 1, 1, 1)
    kind = rec[:, 1].view(B, 1, 1, 1)
    y0, y1, x0, x1 = (rec[:, k].view(B, 1, 1, 1) for k in (2, 3, 4, 5))
    hh = torch.arange(H, device=x.device).view(1, 1, H, 1)
    ww = torch.arange(W, device=x.device).view(1, 1, 1, W)
    box = (hh >= y0) & (hh < y1) & (ww >= x0) & (ww < x1)
    other = x.flip(0)
    blend = (lam * x.float() + (1.0 - lam) * other.float()).to(x.dtype)
    blend = torch.where(x == other, x, blend)
    return torch.where(kind == 1, blend, torch.where((kind == 2) & box, other, x))


class Mixup(nn.Module):
    """``x_mixed, target = Mixup(...)(x, y)`` for ``x [B, C, H, W]`` and class indices ``y [B]``.

    ``mixup_alpha`` / ``cutmix_alpha``: the Beta(alpha, alpha) parameters, 0 switches that kind off.  ``prob``: the
    probability that a batch (``mode="batch"``) or a sample (``mode="elem"``) is mixed at all.  ``switch_prob``: with
    both kinds on, the probability of cutmix.  In ``eval()`` or with both alphas 0 the call returns ``x`` itself and
    a target with ``lam = 1`` and launches nothing.  The images carry no gradient through the mix (it is input
    augmentation).  GPU images must be bf16 or fp32; there is no ATen fallback on the GPU."""

    def __init__(self, mixup_alpha: float = 1.0, cutmix_alpha: float = 0.0, prob: float = 1.0,
                 switch_prob: float = 0.5, mode: str = "batch"):
        super().__init__()
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError(f"Mixup: alphas must not be negative, got {mixup_alpha} and {cutmix_alpha}")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"Mixup: prob and switch_prob must be in [0, 1], got {prob} and {switch_prob}")
        if mode not in ("batch", "elem"):
            raise ValueError(f"Mixup: mode must be 'batch' or 'elem', got {mode!r} (timm's 'pair' is not supported)")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode = float(prob), float(switch_prob), mode

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, MixedTarget]:
        if x.dim() != 4:
            raise ValueError(f"Mixup: expected x [B, C, H, W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        if y.dim() != 1 or y.shape[0] != B:
            raise ValueError(f"Mixup: expected {B} class indices, got {tuple(y.shape)}")
        if not self.training or (self.mixup_alpha == 0 and self.cutmix_alpha == 0):
            return x, MixedTarget(y, y, _one(x.device))
        R = B if self.mode == "elem" else 1
        cfg = (self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob)
        if not x.is_cuda:
            rec = cpu_records(R, H, W, *cfg)
            return mix_reference(x, rec), MixedTarget(y, y.flip(0), lam_of(rec))
        if x.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"ringdp.data.Mixup: the GPU kernel takes bf16 or fp32 images, got {x.dtype} "
                            "(there is no ATen fallback on the GPU)")
        from .._native import C
        from ..random import Draw

        rec = C.mix_draw(Draw(x.device).snapshot, R, H, W, *cfg)
        out, y_b = mix_batch(x, y, rec)
        return out, MixedTarget(y, y_b, lam_of(rec))

    def extra_repr(self) -> str:
        return (f"mixup_alpha={self.mixup_alpha}, cutmix_alpha={self.cutmix_alpha}, prob={self.prob}, "
                f"switch_prob={self.switch_prob}, mode={self.mode!r}")
