"""ringdp.nn - loss modules backed by ringdp kernels on GPU (ATen on CPU); ``ringdp.nn.utils``: gradient clipping."""
from __future__ import annotations

import torch.nn as _nn

from ..ops.dropout import dropout
from ..ops.loss import cross_entropy
from . import utils  # noqa: F401  (ringdp.nn.utils.clip_grad_norm_)


class CrossEntropyLoss(_nn.Module):
    """Drop-in for ``torch.nn.CrossEntropyLoss`` (ref/launch_dist.py:58): fused log-softmax + NLL
    with mean/sum/none reduction, ``ignore_index`` and ``label_smoothing``."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None,
                 reduction: str = "mean", label_smoothing: float = 0.0):
        super().__init__()
        if weight is not None:
            raise NotImplementedError("ringdp.nn.CrossEntropyLoss: per-class weights are not supported")
        if size_average is not None or reduce is not None:
            raise NotImplementedError("ringdp.nn.CrossEntropyLoss: legacy size_average/reduce are not supported")
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing

    def forward(self, input, target):
        return cross_entropy(input, target, self.ignore_index, self.label_smoothing, self.reduction)


class Dropout(_nn.Module):
    """Drop-in for ``torch.nn.Dropout`` on bf16 GPU rows (``ringdp.ops.dropout``): counter-based masks from the
    device-resident ``ringdp.random`` state, regenerated in the backward (no stored mask), hipGraph-safe.  CPU
    tensors go to ATen; other dtypes on the GPU raise.  One difference on the GPU: ``p`` is quantised to a 16-bit
    threshold clamped to 65535, so ``p = 1`` keeps each element with probability 2^-16 (scaled by 65536) where ATen
    zeroes everything; every ``p <= 1 - 2^-16`` is realised to within 2^-17."""

    def __init__(self, p: float = 0.5, inplace: bool = False):
        super().__init__()
        if inplace:
            raise NotImplementedError("ringdp.nn.Dropout: inplace is not supported")
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
        self.p = p

    def forward(self, input, draw=None):
        return dropout(input, self.p, self.training, draw)

    def extra_repr(self) -> str:
        return f"p={self.p}"


__all__ = ["CrossEntropyLoss", "Dropout", "cross_entropy", "dropout"]
