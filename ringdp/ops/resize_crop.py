"""Random-resized-crop, bilinear resize, flip, normalise and random erasing of a uint8 dataset on ringdp's kernels
(``csrc/kernels/resize_crop.hip``): what ``DeviceLoader(resize=S)`` runs.

What happens to a sample is a device record, one per sample or one for the batch, ``int32 [R, 8]``:

====  ==========================================================================
word  content
====  ==========================================================================
0-3   crop box in source pixels ``y0, x0, h, w`` (``1 <= h <= H``, ``1 <= w <= W``, inside the image)
4     flip (0 / 1)
5     erase rows ``ey0 | ey1 << 16`` (half-open, output coordinates; empty box = no erase)
6     erase columns ``ex0 | ex1 << 16``
7     0
====  ==========================================================================

**The image kernel** (``C.resize_crop``).  With ``crop = x[idx[b]][y0:y0+h, x0:x0+w]`` the output of sample ``b`` is
``F.interpolate(crop, (S, S), mode="bilinear", align_corners=False, antialias=False)`` - half-pixel centres, source
indices clamped to the box: ``s = (h / S) * (oy + 0.5) - 0.5`` clamped at 0, rows ``floor(s)`` and
``min(floor(s) + 1, h - 1)``, weight ``s - floor(s)``, the same in x - then mirrored in x if flip is set, mapped to
``(v / 255 - mean[c]) / std[c]`` (evaluated as one fma, ``v * (inv_std[c] / 255) - mean[c] * inv_std[c]``), set to 0
inside the erase box and rounded once to bf16 or fp32.  Arithmetic is fp32.  A box larger than ``S`` is shrunk by the same plain bilinear rule: there is no antialiasing filter.  The
kernel clamps a record's box into the image, so a record made by hand cannot make it read out of bounds.  A source
image may have up to 32 KiB (``H * W * C``, staged in LDS) and ``S`` may be up to 1024.

**The draw kernel** (``C.crop_draw``), one thread per record, torchvision's ``RandomResizedCrop.get_params``,
``RandomHorizontalFlip`` and ``RandomErasing.get_params`` (value 0) in fp32.  Every generator call is Philox4x32-10
of an ``rng_tick`` snapshot (``ringdp.random.Draw``): key = seed, counter = ``(record, step lo, step hi, round)``;
a uniform is ``(word >> 8) * 2**-24`` of the call's words ``u0..u3``.

* rounds 0..9, crop attempt ``t`` (skipped with ``scale=None``: the whole image)
  ``area = H * W * (s0 + (s1 - s0) * u0)``, ``ar = exp(ln r0 + (ln r1 - ln r0) * u1)``,
  ``w = rint(sqrt(area * ar))``, ``h = rint(sqrt(area / ar))``; the first attempt with ``1 <= w <= W`` and
  ``1 <= h <= H`` is taken, with ``y0 = floor(u2 * (H - h + 1))`` and ``x0 = floor(u3 * (W - w + 1))`` (clamped).
  If none of the ten fits: the centre crop with the image's own ratio clamped to ``[r0, r1]`` - ``w = W, h =
  rint(W / r0)`` when ``W / H < r0``, ``h = H, w = rint(H * r1)`` when ``W / H > r1``, else the whole image.
* round 10  flip iff ``hflip`` and ``u0 < 0.5``; erase iff ``u1 < erase_prob``
* rounds 11..20, erase attempt ``t`` on the ``S x S`` output
  ``area = S * S * (e0 + (e1 - e0) * u0)``, ``ar = exp(ln q0 + (ln q1 - ln q0) * u1)``,
  ``eh = rint(sqrt(area * ar))``, ``ew = rint(sqrt(area / ar))``; the first attempt with ``eh < S`` and ``ew < S``
  is taken, at ``ey0 = floor(u2 * (S - eh + 1))``, ``ex0 = floor(u3 * (S - ew + 1))``.  If none fits (or the box
  has no rows or columns) the erase box is empty.  timm's per-pixel-noise mode is not provided.

Both loops are bounded, and a captured step (``StepGraph``) draws new boxes on every replay.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .._native import C

Range = Tuple[float, float]


def _range(v, name: str) -> Range:
    lo, hi = (float(t) for t in v)
    if not 0.0 < lo <= hi:
        raise ValueError(f"{name}: expected 0 < lo <= hi, got ({lo}, {hi})")
    return lo, hi


def crop_records(snapshot: torch.Tensor, R: int, H: int, W: int, S: int, scale: Optional[Range] = (0.08, 1.0),
                 ratio: Range = (3 / 4, 4 / 3), hflip: bool = False, erase_prob: float = 0.0,
                 erase_scale: Range = (0.02, 0.33), erase_ratio: Range = (0.3, 3.3)) -> torch.Tensor:
    """``R`` records ``int32 [R, 8]`` for source images ``H x W`` and output ``S x S``, drawn on the device from an
    ``rng_tick`` snapshot as the module docstring defines.  ``scale=None``: no random crop, the whole image."""
    if not 0.0 <= erase_prob <= 1.0:
        raise ValueError(f"crop_records: erase_prob must be in [0, 1], got {erase_prob}")
    return C.crop_draw(snapshot, int(R), int(H), int(W), int(S),
                       None if scale is None else _range(scale, "crop_records scale"),
                       _range(ratio, "crop_records ratio"), bool(hflip), float(erase_prob),
                       _range(erase_scale, "crop_records erase_scale"),
                       _range(erase_ratio, "crop_records erase_ratio"))


def whole_image_record(H: int, W: int, device) -> torch.Tensor:
    """The one static record ``[1, 8]`` of the evaluation transform: the whole image, no flip, no erase."""
    return torch.tensor([[0, 0, H, W, 0, 0, 0, 0]], dtype=torch.int32).to(device)


def resize_crop(x: torch.Tensor, labels: Optional[torch.Tensor], idx: torch.Tensor, rec: torch.Tensor, size: int,
                mean: Sequence[float] = (), std: Sequence[float] = (), channels_last: bool = False,
                out_dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``(images [B, C, size, size], labels[idx])`` from the GPU-resident uint8 dataset ``x [N, H, W]`` or
    ``[N, H, W, C]``, batch indices ``idx`` int64 ``[B]`` and records ``int32 [1, 8]`` (one for the batch) or
    ``[B, 8]``.  ``channels_last=True`` gives the channels-last memory format.  One launch; no ATen fallback."""
    if not x.is_cuda:
        raise RuntimeError("ringdp.ops.resize_crop: expected a GPU-resident dataset (ringdp.data.transforms has the "
                           "CPU path)")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"ringdp.ops.resize_crop: the kernel writes bf16 or fp32, got {out_dtype}")
    out, y = C.resize_crop(x, labels, idx, rec, int(size), list(mean), list(std), bool(channels_last), out_dtype)
    return out, (y if labels is not None else None)


__all__ = ["crop_records", "whole_image_record", "resize_crop"]
