"""Train-time image augmentation for the folder loaders (K25): random resized crop, horizontal flip and colour jitter, sampled
on the host and applied on the device by ``image_to_graph.crop_resize`` and ``image_to_graph.color_jitter`` (csrc/augment.hip),
whose pixels are Pillow's byte for byte.

``Augmentation`` only draws parameters.  ``GraphImageFolder(..., augment=Augmentation(...))`` and ``ImageTensorFolder(...,
augment=...)`` hand them to ``graphs_from_images`` / ``tensors_from_images`` chunk by chunk.

The parameters are those of torchvision's ``RandomResizedCrop``, ``RandomHorizontalFlip`` and ``ColorJitter``, and the crop
follows torchvision's rule.  torchvision is not a dependency of this package and its random stream is NOT reproduced: the same
seed gives other crops than ``torchvision.transforms`` would draw.  Hue jitter is out of scope (Pillow has no enhancer for it;
torchvision's goes through an HSV round trip of its own).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

# the six orders of (0 brightness, 1 contrast, 2 saturation); one is drawn per image, as ColorJitter permutes its operations
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TRIES = 10                    # RandomResizedCrop's attempts before the central fallback
_DRAWS = 2 * TRIES + 2 + 1 + 3 + 1  # uniforms per sample: tries, crop position, flip, three factors, order


class AugmentParams(NamedTuple):
    """Host arrays for a list of images: what ``crop_resize`` and ``color_jitter`` take."""
    boxes: np.ndarray                  # int64 [B, 4]: left, top, right, bottom
    flips: np.ndarray                  # bool [B]
    brightness: Optional[np.ndarray]   # float32 [B], or None when that jitter is off
    contrast: Optional[np.ndarray]
    saturation: Optional[np.ndarray]
    order: np.ndarray                  # int32 [B, 3]: a row of ORDERS per image


def _mix(seed: int, epoch: int, index: int) -> int:
    """(seed, epoch, sample index) -> one 63-bit generator seed (splitmix64's finaliser over the three words)"""
    z = 0
    for word in (seed, epoch, index):
        z = (z + (int(word) & 0xFFFFFFFFFFFFFFFF) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 31
    return z & 0x7FFFFFFFFFFFFFFF


def _jitter_range(value, name: str):
    """ColorJitter's argument check: an amount a gives [max(0, 1 - a), 1 + a], a (lo, hi) pair is taken as given; None when the
    range is the single point 1 (no operation)."""
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError(f"{name} must be non-negative, got {value}")
        lo, hi = max(0.0, 1.0 - float(value)), 1.0 + float(value)
    else:
        lo, hi = (float(v) for v in value)
        if not 0.0 <= lo <= hi:
            raise ValueError(f"{name} must be a range 0 <= lo <= hi, got {tuple(value)}")
    return None if lo == hi == 1.0 else (lo, hi)


def central_crop(height: int, width: int, ratio) -> tuple:
    """RandomResizedCrop's fallback: the whole image, or its centre at the nearest allowed aspect ratio.  (left, top, right, bottom)"""
    in_ratio = width / height
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    w, h = min(max(w, 1), width), min(max(h, 1), height)
    top, left = (height - h) // 2, (width - w) // 2
    return left, top, left + w, top + h


class Augmentation:
    """``Augmentation(scale=(0.08, 1.0), ratio=(3/4, 4/3), hflip=0.5, brightness=0.0, contrast=0.0, saturation=0.0, seed=0)``.

    ``scale`` / ``ratio``: ``RandomResizedCrop``'s area fraction and aspect-ratio ranges (``scale=None``: no crop, the whole image is
    resized).  ``hflip``: the probability of ``RandomHorizontalFlip`` (0: never).  ``brightness`` / ``contrast`` / ``saturation``:
    ``ColorJitter``'s arguments - an amount ``a`` draws the factor uniformly from ``[max(0, 1 - a), 1 + a]``, a ``(lo, hi)`` pair is
    taken as given, 0 switches the operation off; the operations run in a random order per image.  No hue (see the module text).

    The draws of a sample come from a PRIVATE ``torch.Generator`` seeded from ``(seed, epoch, sample index)`` alone.  So a sample's
    parameters do not depend on the loader's chunk, batch size, workers or shuffle, a run can be repeated, and the global RNG -
    from which the loaders draw their order as a ``DataLoader`` does - is never touched.  torchvision's random stream is not
    reproduced."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), hflip=0.5, brightness=0.0, contrast=0.0, saturation=0.0,
                 seed=0):
        if scale is not None:
            scale = (float(scale[0]), float(scale[1]))
            if not 0.0 < scale[0] <= scale[1]:
                raise ValueError(f"scale must be a range 0 < lo <= hi, got {scale}")
        ratio = (float(ratio[0]), float(ratio[1]))
        if not 0.0 < ratio[0] <= ratio[1]:
            raise ValueError(f"ratio must be a range 0 < lo <= hi, got {ratio}")
        if not 0.0 <= float(hflip) <= 1.0:
            raise ValueError(f"hflip must be a probability, got {hflip}")
        self.scale, self.ratio, self.hflip, self.seed = scale, ratio, float(hflip), int(seed)
        self.brightness = _jitter_range(brightness, "brightness")
        self.contrast = _jitter_range(contrast, "contrast")
        self.saturation = _jitter_range(saturation, "saturation")

    def _uniforms(self, epoch: int, index: int) -> np.ndarray:
        g = torch.Generator()
        g.manual_seed(_mix(self.seed, epoch, index))
        return torch.rand(_DRAWS, dtype=torch.float64, generator=g).numpy()

    def _box(self, height: int, width: int, u: np.ndarray) -> tuple:
        """torchvision's ``RandomResizedCrop.get_params``: ten tries of (area, log-uniform ratio), the first that fits at a uniform
        position; else the central crop at the clamped ratio."""
        if self.scale is None:
            return 0, 0, width, height
        area = height * width
        log_lo, log_hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        for t in range(TRIES):
            target = area * (self.scale[0] + (self.scale[1] - self.scale[0]) * u[2 * t])
            aspect = math.exp(log_lo + (log_hi - log_lo) * u[2 * t + 1])
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                top = min(int(u[2 * TRIES] * (height - h + 1)), height - h)
                left = min(int(u[2 * TRIES + 1] * (width - w + 1)), width - w)
                return left, top, left + w, top + h
        return central_crop(height, width, self.ratio)

    def sample(self, sizes, epoch: int, indices) -> AugmentParams:
        """The parameters of the images ``indices`` (their ``(height, width)`` in ``sizes``) in epoch ``epoch``, as host arrays."""
        sizes, indices = list(sizes), [int(i) for i in indices]
        if len(sizes) != len(indices):
            raise ValueError(f"sample: {len(sizes)} sizes for {len(indices)} indices")
        B = len(indices)
        boxes = np.zeros((B, 4), np.int64)
        flips = np.zeros(B, bool)
        factors = np.ones((B, 3), np.float32)
        order = np.zeros((B, 3), np.int32)
        ranges = (self.brightness, self.contrast, self.saturation)
        at = 2 * TRIES + 2
        for b, ((h, w), index) in enumerate(zip(sizes, indices)):
            if h < 1 or w < 1:
                raise ValueError(f"sample: empty image {h} x {w}")
            u = self._uniforms(int(epoch), index)
            boxes[b] = self._box(int(h), int(w), u)
            flips[b] = u[at] < self.hflip
            for op, r in enumerate(ranges):
                if r is not None:
                    factors[b, op] = np.float32(r[0] + (r[1] - r[0]) * u[at + 1 + op])
            order[b] = ORDERS[min(int(u[at + 4] * len(ORDERS)), len(ORDERS) - 1)]
        given = [factors[:, op].copy() if r is not None else None for op, r in enumerate(ranges)]
        return AugmentParams(boxes, flips, given[0], given[1], given[2], order)
