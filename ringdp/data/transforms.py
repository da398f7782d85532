"""Host-side image transforms on uint8 tensors (torchvision-compatible semantics).

The reference pipelines:
  W1  ``Compose([ToTensor(), Normalize((0.1307,), (0.3081,))])``       ref/launch_dist.py:64-65
  W2  ``Compose([RandomCrop(32, padding=4), RandomHorizontalFlip(), ToTensor(),
                 Normalize((0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010))])``  ref/example_mp.py:56-70

Images are uint8 tensors, (H, W) for grayscale or (H, W, C) channels-last as stored on disk.
``ToTensor`` produces float32 CHW in [0, 1] exactly like torchvision.  The same transforms run on
the GPU inside the device loader (``ringdp.data.device_loader``: one fused HIP kernel for
gather + crop + flip + normalise); these host versions are the reference semantics and the CPU path.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch


class Compose:
    def __init__(self, transforms: Sequence[Callable]):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x

    def __repr__(self) -> str:
        return "Compose(" + ", ".join(repr(t) for t in self.transforms) + ")"


def _hwc(img: torch.Tensor) -> torch.Tensor:
    return img.unsqueeze(-1) if img.dim() == 2 else img


class ToTensor:
    """uint8 (H, W[, C]) -> float32 (C, H, W) / 255."""

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        if img.dtype != torch.uint8:
            raise TypeError("ToTensor expects a uint8 image")
        return _hwc(img).permute(2, 0, 1).contiguous().to(torch.float32).div_(255.0)

    def __repr__(self) -> str:
        return "ToTensor()"


class Normalize:
    def __init__(self, mean: Sequence[float], std: Sequence[float], inplace: bool = False):
        self.mean = tuple(float(m) for m in mean)
        self.std = tuple(float(s) for s in std)
        if any(s == 0 for s in self.std):
            raise ValueError("Normalize: std must be non-zero")
        self.inplace = inplace

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        if not self.inplace:
            t = t.clone()
        m = torch.tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        s = torch.tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.sub_(m).div_(s)

    def __repr__(self) -> str:
        return f"Normalize(mean={self.mean}, std={self.std})"


class RandomCrop:
    """Zero-pad by ``padding`` then crop ``size`` at a uniformly random offset (uint8 HW[C])."""

    def __init__(self, size, padding: int = 0, generator: Optional[torch.Generator] = None):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.padding = int(padding)
        self.generator = generator

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        x = _hwc(img)
        p = self.padding
        if p:
            x = torch.nn.functional.pad(x.permute(2, 0, 1), (p, p, p, p)).permute(1, 2, 0)
        H, W = x.shape[0], x.shape[1]
        th, tw = self.size
        i = int(torch.randint(0, H - th + 1, (1,), generator=self.generator))
        j = int(torch.randint(0, W - tw + 1, (1,), generator=self.generator))
        out = x[i:i + th, j:j + tw]
        return out.squeeze(-1) if img.dim() == 2 else out.contiguous()

    def __repr__(self) -> str:
        return f"RandomCrop(size={self.size}, padding={self.padding})"


class RandomHorizontalFlip:
    def __init__(self, p: float = 0.5, generator: Optional[torch.Generator] = None):
        self.p = float(p)
        self.generator = generator

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        if float(torch.rand((), generator=self.generator)) < self.p:
            return img.flip(1).contiguous()
        return img

    def __repr__(self) -> str:
        return f"RandomHorizontalFlip(p={self.p})"


def _resize_u8(img: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """uint8 HW[C] -> uint8 size[C]: plain bilinear (half-pixel centres, no antialiasing), rounded to nearest."""
    if img.dtype != torch.uint8:
        raise TypeError("resize expects a uint8 image")
    t = _hwc(img).permute(2, 0, 1).unsqueeze(0).to(torch.float32)
    t = torch.nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False, antialias=False)
    out = t.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
    return out.squeeze(-1) if img.dim() == 2 else out.contiguous()


def _size2(size) -> Tuple[int, int]:
    size = (size, size) if isinstance(size, int) else tuple(int(s) for s in size)
    if len(size) != 2 or min(size) < 1:
        raise ValueError(f"size must be a positive int or a pair of them, got {size}")
    return size


class Resize:
    """Bilinear resize of a uint8 HW[C] image to ``size`` (an int means ``size x size``), the definition the device
    loader's ``resize`` uses (``ringdp.ops.resize_crop``); the result is rounded back to uint8 for ``ToTensor``."""

    def __init__(self, size):
        self.size = _size2(size)

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        return _resize_u8(img, self.size)

    def __repr__(self) -> str:
        return f"Resize(size={self.size})"


class RandomResizedCrop:
    """torchvision's ``RandomResizedCrop`` on a uint8 HW[C] image: ten attempts at a box of ``scale`` x the area
    and a log-uniform ``ratio``, else the centre crop with the ratio clamped; the box is resized like ``Resize``."""

    def __init__(self, size, scale: Sequence[float] = (0.08, 1.0), ratio: Sequence[float] = (3 / 4, 4 / 3),
                 generator: Optional[torch.Generator] = None):
        self.size = _size2(size)
        self.scale = tuple(float(s) for s in scale)
        self.ratio = tuple(float(r) for r in ratio)
        if not 0 < self.scale[0] <= self.scale[1] or not 0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError(f"RandomResizedCrop: expected 0 < lo <= hi, got scale {self.scale}, ratio {self.ratio}")
        self.generator = generator

    def get_params(self, H: int, W: int) -> Tuple[int, int, int, int]:
        """The box ``(y0, x0, h, w)`` for an ``H x W`` image."""
        import math

        lr0, lr1 = math.log(self.ratio[0]), math.log(self.ratio[1])
        for _ in range(10):
            u = torch.rand(2, generator=self.generator).tolist()
            area = H * W * (self.scale[0] + (self.scale[1] - self.scale[0]) * u[0])
            ar = math.exp(lr0 + (lr1 - lr0) * u[1])
            w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if 1 <= w <= W and 1 <= h <= H:
                y0 = int(torch.randint(0, H - h + 1, (1,), generator=self.generator))
                x0 = int(torch.randint(0, W - w + 1, (1,), generator=self.generator))
                return y0, x0, h, w
        h, w = H, W
        if W / H < self.ratio[0]:
            h = min(max(int(round(W / self.ratio[0])), 1), H)
        elif W / H > self.ratio[1]:
            w = min(max(int(round(H * self.ratio[1])), 1), W)
        return (H - h) // 2, (W - w) // 2, h, w

    def __call__(self, img: torch.Tensor) -> torch.Tensor:
        y0, x0, h, w = self.get_params(img.shape[0], img.shape[1])
        return _resize_u8(img[y0:y0 + h, x0:x0 + w], self.size)

    def __repr__(self) -> str:
        return f"RandomResizedCrop(size={self.size}, scale={self.scale}, ratio={self.ratio})"


def default_collate(batch: List[Tuple[object, object]]):
    """Stack (image, target) pairs into (images, targets) tensors."""
    xs, ys = zip(*batch)
    x = torch.stack([torch.as_tensor(v) for v in xs])
    y = torch.as_tensor(ys, dtype=torch.int64)
    return x, y
