"""Mixup / CutMix on ringdp's kernels (``csrc/kernels/mixup.hip``) and the cross entropy of the mixed targets
(``ce_mix_*`` in ``csrc/kernels/elementwise.hip``).

A mixed batch pairs sample ``b`` with sample ``B - 1 - b`` (timm's ``flip(0)``).  What is mixed, and how much, is a
device record per batch or per sample, ``int32 [R, 8]``:

====  ==========================================================================
word  content
====  ==========================================================================
0     ``lam`` (fp32 bits): the weight of the sample's own label
1     kind: 0 not applied, 1 mixup, 2 cutmix
2-5   box ``y0, y1, x0, x1`` (half-open; empty for kinds 0 and 1)
6     ``lam0`` (fp32 bits): the Beta(alpha, alpha) draw before the box correction
7     0
====  ==========================================================================

* kind 1  ``out = lam * x[b] + (1 - lam) * x[B-1-b]`` (fp32 fma, rounded once to the output type)
* kind 2  ``out = x[B-1-b]`` inside the box, ``x[b]`` outside (a bit copy); ``lam = 1 - box area / (H * W)``
* kind 0  ``out = x[b]`` bit for bit, ``lam = 1``

``C.mix_draw`` fills the records from an ``rng_tick`` snapshot (``ringdp.random.Draw``) with Philox4x32-10,
key = seed, counter = ``(record, step lo, step hi, round)``, so a captured step draws a new ``lam`` and box on
every replay; ``ringdp.data.Mixup`` is the user-facing transform.  ``lam0`` is sampled on the device in fp32 as a
ratio of two Marsaglia-Tsang gamma variates (``alpha == 1``: the uniform itself); each variate's rejection loop stops
after 8 attempts, which refuses a proper sample with probability below 4e-11, and keeps its last candidate then.  The loss reads ``lam`` straight from word 0 of
the records (a strided view): nothing that changes from step to step passes through the host.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F

from .._native import C

_RED = {"none": 0, "mean": 1, "sum": 2}


class MixedTarget:
    """The labels of a mixed batch: ``y_a`` with weight ``lam`` and ``y_b`` with weight ``1 - lam``.  ``lam`` is an
    fp32 tensor of shape ``[1]`` (one value for the batch) or ``[B]``, of any stride - normally a view of word 0 of
    the mixup records."""

    __slots__ = ("y_a", "y_b", "lam")

    def __init__(self, y_a: torch.Tensor, y_b: torch.Tensor, lam: torch.Tensor):
        if y_a.dim() != 1 or y_b.shape != y_a.shape:
            raise ValueError(f"MixedTarget: y_a and y_b must be 1-D and alike, got {tuple(y_a.shape)} and "
                             f"{tuple(y_b.shape)}")
        if lam.dtype != torch.float32 or lam.dim() != 1 or lam.shape[0] not in (1, y_a.shape[0]):
            raise ValueError(f"MixedTarget: lam must be an fp32 tensor of shape [1] or [{y_a.shape[0]}], got "
                             f"{lam.dtype} {tuple(lam.shape)}")
        self.y_a, self.y_b, self.lam = y_a, y_b, lam

    def dense(self, num_classes: int, label_smoothing: float = 0.0) -> torch.Tensor:
        """The ``[B, C]`` fp32 probability matrix ``(1 - s) * (lam * onehot(y_a) + (1 - lam) * onehot(y_b)) + s / C``
        - for references and the CPU path; the GPU loss never builds it."""
        lam = self.lam.reshape(-1, 1)
        q = lam * F.one_hot(self.y_a.long(), num_classes).float() \
            + (1.0 - lam) * F.one_hot(self.y_b.long(), num_classes).float()
        if label_smoothing:
            q = (1.0 - label_smoothing) * q + label_smoothing / num_classes
        return q


class MixedCrossEntropyF(torch.autograd.Function):
    """Cross entropy of fp32 logits ``[B, C]`` against a ``MixedTarget`` on the GPU; gradient for the logits only."""

    @staticmethod
    def forward(ctx, logits, y_a, y_b, lam, label_smoothing: float, reduction: str):
        logits = logits.float().contiguous()
        y_a, y_b = y_a.long().contiguous(), y_b.long().contiguous()
        loss, lse, ws = C.cross_entropy_mix_fwd(logits, y_a, y_b, lam, label_smoothing, _RED[reduction])
        ctx.save_for_backward(logits, y_a, y_b, lam, lse, ws)
        ctx.cfg = (label_smoothing, _RED[reduction])
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        logits, y_a, y_b, lam, lse, ws = ctx.saved_tensors
        d = C.cross_entropy_mix_bwd(logits, y_a, y_b, lam, lse, ws, grad_out.contiguous(), *ctx.cfg)
        return d, None, None, None, None, None


def mixed_cross_entropy(logits: torch.Tensor, target: MixedTarget, label_smoothing: float = 0.0,
                        reduction: str = "mean") -> torch.Tensor:
    """``sum_c -q[r, c] * log_softmax(logits)[r, c]`` with ``q = target.dense(C, label_smoothing)``; every row
    counts, so ``mean`` divides by ``B``.  GPU logits run ringdp's kernels (no model-head fusion), CPU logits ATen."""
    if reduction not in _RED:
        raise ValueError(f"mixed_cross_entropy: unknown reduction {reduction!r}")
    if logits.dim() != 2 or logits.shape[0] != target.y_a.shape[0]:
        raise ValueError(f"mixed_cross_entropy: expected logits [B, C] with B = {target.y_a.shape[0]}, got "
                         f"{tuple(logits.shape)}")
    if logits.is_cuda:
        return MixedCrossEntropyF.apply(logits, target.y_a, target.y_b, target.lam, float(label_smoothing), reduction)
    return F.cross_entropy(logits, target.dense(logits.shape[1]).to(logits.dtype), label_smoothing=label_smoothing,
                           reduction=reduction)


def mix_batch(x: torch.Tensor, y: torch.Tensor, rec: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(x mixed as the records say, y.flip(0))`` for a GPU batch ``x [B, C, H, W]`` (bf16 or fp32, NCHW or
    channels-last) and records ``int32 [1, 8]`` or ``[B, 8]``.  The result is a fresh tensor in ``x``'s layout;
    ``x`` is not written.  This is input augmentation: no gradient flows back to ``x``."""
    if x.dim() != 4:
        raise ValueError(f"mix_batch: expected x [B, C, H, W], got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("ringdp.ops.mixup.mix_batch: expected a GPU tensor (ringdp.data.Mixup has the CPU path)")
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"ringdp.ops.mixup.mix_batch: the GPU kernel takes bf16 or fp32, got {x.dtype} "
                        "(there is no ATen fallback on the GPU)")
    x = x.detach()
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        x = x.contiguous()
    out, y_b = C.mix_images(x, y.long().contiguous(), rec)
    return out, y_b


def lam_of(rec: torch.Tensor) -> torch.Tensor:
    """Word 0 of the records as an fp32 view ``[R]`` with stride 8: what ``MixedTarget`` carries."""
    return rec.view(torch.float32)[:, 0]


__all__ = ["MixedTarget", "MixedCrossEntropyF", "mixed_cross_entropy", "mix_batch", "lam_of"]
