"""Classification loss on the device (DESIGN K23): ``ClassificationLoss`` is a drop-in for the ``criterion`` every step and capture
class takes.  One launch of ``csrc/class_loss.hip`` gives the loss, its gradient, the trainer's float64 loss accumulator, the
confusion counts and a label check - so a captured step reports accuracy and a confusion matrix without a host read per step.
"""
from __future__ import annotations

import math
import numbers

import torch
import torch.nn as nn

from . import functional as Fn
from . import native

LOSS_OPTION_DEFAULTS = dict(class_weight=None, label_smoothing=0.0, pos_weight=None)


def check_loss_options(kind: str = "ce", class_weight=None, label_smoothing: float = 0.0, pos_weight=None,
                       reduction: str = "mean") -> None:
    """ValueError for an unknown name or values that do not go together.  Touches no device."""
    finite = lambda v: isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)  # noqa: E731
    if kind not in native.LOSS_KINDS:
        raise ValueError(f"loss kind {kind!r}: one of {sorted(native.LOSS_KINDS)} expected")
    if reduction not in native.LOSS_REDUCTIONS:
        raise ValueError(f"loss reduction {reduction!r}: one of {sorted(native.LOSS_REDUCTIONS)} expected")
    if not (finite(label_smoothing) and 0.0 <= label_smoothing < 1.0):
        raise ValueError(f"label_smoothing {label_smoothing!r}: a value in [0, 1) expected")
    if class_weight is not None:
        if kind == "bce":
            raise ValueError("class_weight belongs to kind='ce'; the binary loss takes pos_weight")
        values = class_weight.tolist() if isinstance(class_weight, torch.Tensor) else list(class_weight)
        if not values or not all(finite(v) and v >= 0 for v in values):
            raise ValueError(f"class_weight {values!r}: finite values >= 0, one per class, expected")
    if pos_weight is not None:
        if kind == "ce":
            raise ValueError("pos_weight belongs to kind='bce'; the cross-entropy takes class_weight")
        if not (finite(pos_weight) and pos_weight >= 0):
            raise ValueError(f"pos_weight {pos_weight!r}: a finite value >= 0 expected")


class ClassificationLoss(nn.Module):
    """``criterion(logits, labels, scale=1.0) -> 0-dim loss`` on ``functional.class_loss``.

    ``kind="ce"``: ``nn.CrossEntropyLoss(weight=class_weight, label_smoothing=..., reduction=...)`` on logits ``[G, C]`` (or ``[C]``
    with a 0-dim label).  ``kind="bce"``: the write-up's binary cross-entropy on ONE logit per sample, labels 0 / 1, targets smoothed
    to ``y (1 - s) + s / 2``, positives weighted by ``pos_weight``.  ``scale`` multiplies the loss and its gradient inside the launch.

    The module owns the device ``status`` word (bit 0: a label outside the classes was seen; such a sample is left out of the loss,
    the gradient and the counts - ``check()`` reads the word and raises IndexError).  With ``track_metrics`` it owns ``confusion``,
    int64 ``[K, K]`` with rows = true class (K = C, or 2 for "bce"), allocated at the first call and counted up by every call -
    training calls included, replays of a captured step too; ``reset_metrics()`` clears it.  ``bind_loss_sum(t)`` makes every call
    add its loss to ``t`` (float64, one element) inside the launch: the trainer's epoch accumulator.  ``state_snapshot()`` /
    ``state_restore()`` cover the counts and the status word (a capture's warm-up must not count)."""

    def __init__(self, kind: str = "ce", class_weight=None, label_smoothing: float = 0.0, pos_weight: float | None = None,
                 reduction: str = "mean", track_metrics: bool = False):
        check_loss_options(kind, class_weight, label_smoothing, pos_weight, reduction)
        super().__init__()
        self.kind, self.label_smoothing, self.reduction = kind, float(label_smoothing), reduction
        self.pos_weight = 1.0 if pos_weight is None else float(pos_weight)
        self.track_metrics = bool(track_metrics)
        self._class_weight = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32).reshape(-1).clone()
        self.class_weight = None  # the device copy, made at the first call
        self.status = self.confusion = self.loss_sum = self._workspace = None
        self.num_classes = None   # K

    def bind_loss_sum(self, loss_sum: torch.Tensor | None) -> "ClassificationLoss":
        if loss_sum is not None and (loss_sum.dtype != torch.float64 or loss_sum.numel() != 1):
            raise ValueError("bind_loss_sum: one float64 element expected")
        self.loss_sum = loss_sum
        return self

    def accumulates_into(self, loss_sum: torch.Tensor) -> bool:
        """True when every call already adds its loss to ``loss_sum`` (the caller then skips its own accumulate)."""
        return self.loss_sum is not None and self.loss_sum.data_ptr() == loss_sum.data_ptr()

    def _prepare(self, logits: torch.Tensor) -> None:
        C = int(logits.size(-1))
        if self.kind == "bce" and C != 1:
            raise ValueError(f"ClassificationLoss(kind='bce') takes ONE logit per sample, the model gives {C}")
        if self._class_weight is not None and self._class_weight.numel() != C:
            raise ValueError(f"class_weight has {self._class_weight.numel()} entries, the model gives {C} classes")
        K = 2 if self.kind == "bce" else C
        if self.num_classes is not None and (K != self.num_classes or self.status.device != logits.device):
            raise ValueError(f"ClassificationLoss: made for {self.num_classes} classes on {self.status.device}, called with {K} on "
                             f"{logits.device}")
        if self.num_classes is None:
            dev = logits.device
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._workspace = torch.zeros(native.CLASS_LOSS_WORKSPACE_DOUBLES, dtype=torch.float64, device=dev)
            if self._class_weight is not None:
                self.class_weight = self._class_weight.to(dev)
            if self.track_metrics:
                self.confusion = torch.zeros(K, K, dtype=torch.int64, device=dev)
            self.num_classes = K

    def forward(self, logits: torch.Tensor, labels, scale: float = 1.0) -> torch.Tensor:
        self._prepare(logits)
        return Fn.class_loss(logits, labels, kind=self.kind, class_weight=self.class_weight, label_smoothing=self.label_smoothing,
                             pos_weight=self.pos_weight, reduction=self.reduction, scale=scale, status=self.status,
                             loss_sum=self.loss_sum, confusion=self.confusion, workspace=self._workspace)

    def reset_metrics(self) -> None:
        if self.confusion is not None:
            self.confusion.zero_()

    def check(self) -> None:
        """One host read; IndexError when a label outside the classes was seen since the last check (the word is cleared)."""
        if self.status is not None and int(self.status.item()) & 1:
            self.status.zero_()
            raise IndexError(f"ClassificationLoss: a label lies outside the {self.num_classes} classes [0, {self.num_classes})")

    def _state(self):
        return [t for t in (self.status, self.confusion) if t is not None]

    def state_snapshot(self):
        return [t.clone() for t in self._state()]

    def state_restore(self, snap) -> None:
        """Back to ``snap``; tensors made after it was taken (the first call came later) go back to zero."""
        state = self._state()
        for dst, src in zip(state, snap):
            dst.copy_(src)
        for dst in state[len(snap):]:
            dst.zero_()


def accuracy_of(confusion: torch.Tensor) -> float:
    """Share of the diagonal of a confusion matrix (0.0 for an empty one)."""
    total = int(confusion.sum())
    return float(confusion.diagonal().sum()) / total if total else 0.0
