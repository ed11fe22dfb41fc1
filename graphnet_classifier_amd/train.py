"""Training loop of the reference (``utils/train_model.py:8-81``) on the HIP path - SURVEY.md section 8, row f3.

``train(model, dataset, epochs, patience=5, output_path='weights', start_weights=None)`` has the reference's
signature and observable behaviour: Adam(lr=1e-3) (:9), CrossEntropyLoss (:10), one optimizer step per sample in
dataset order (:35-45), average training loss per epoch, early stopping on it (:57-69), ``best_model_epoch{k}.pth``
/ ``final_model.pth`` (:61-62, :72-73) and the timestamped log file with the reference's line formats (:22-30,
:52-54, :76-80).  What differs is how a step runs and how the run is organised:

* parameters and gradients are views of two flat fp32 buffers (``FlatParameters``), the optimizer is ONE fused Adam
  launch over them (``FusedAdam`` -> ``gnc_adam_step_f32``) instead of a walk over 76 tensors;
* AdamW, SGD, gradient clipping by the global norm, learning-rate schedules (``lr_at``) and a skip on non-finite gradients are
  keyword options of ``train()`` (``FusedAdam``'s options, ``FusedSGD``): their scalars live on the device, so a captured step
  replays them (``native.optimizer_ctl_step``, DESIGN K22); the default stays the reference's optimizer;
* ``loss="ce"`` / ``"bce"`` replace ``CrossEntropyLoss`` by the device loss head (``loss.ClassificationLoss``, DESIGN K23): class
  weights, label smoothing or the write-up's binary cross-entropy, with loss, gradient, the loss accumulator, the training
  confusion counts (``metrics=True``) and a label check in ONE launch of the captured step; the default stays the reference's loss;
* the running loss is accumulated on the device (float64 scalar) and read once per epoch, where the reference
  synchronises on ``loss.item()`` after every sample (:44);
* when consecutive samples share one topology (pixel / patch graphs: the edge list depends on the image size only,
  utils/image_to_graph/image_to_graph_optimized.py:42-47) the whole step - forward, loss, backward, gradient pack,
  Adam - is captured into a hipGraph once and replayed per sample (``CapturedTrainStep``): one launch per step
  instead of ~150;
* when every sample brings a NEW topology (superpixel graphs, single or in mini-batches) the step is captured over padded
  buffers that any sample up to a capacity fits; ONE rule, ``_PaddedCaptures``, says when such a capture is made, grown and
  checked, for the training loop and for ``evaluate`` / ``predict``;
* a loader that yields ``(synthetic.GraphBatch, labels [B])`` (``GraphImageFolder.loader(batch_size=B)``) is stepped once per
  mini-batch through ``CombinedModel.forward_batched`` - mean cross-entropy over the batch, captured when consecutive full
  batches share a topology; ``evaluate`` / ``predict`` score a model over either loader form;
* a loader that yields plain tensor batches (``ImageTensorFolder.loader(batch_size=8)``: the reference's image-MLP baseline) is
  stepped once per batch through ``model(x)``, captured when two consecutive batches share their shape (``CapturedTensorStep``);
* the run's side effects live in three small objects: ``RunJournal`` (the log file and the console lines),
  ``PlateauStopper`` (best loss so far, epochs without improvement) and ``CheckpointShelf`` (the ``.pth`` files).

Saved ``.pth`` files hold CPU tensors under the reference's state-dict keys, so they load in the reference as they
are (``utils/inference.py:40-45``) and vice versa.
"""
from __future__ import annotations

import math
import numbers
import os
import time
from datetime import datetime
from typing import Callable, NamedTuple

import torch
import torch.distributed as dist
import torch.nn as nn

from . import native
from .GNN import (CapturedRaggedBatchForward, CombinedModel, FixedGraphFeed, PaddedGraphFeed, RaggedBatchFeed, _Captured,
                  _has_batchnorm, _no_capture_with_pooling, _same_topology, flatten_readout_rows, graph_logits,
                  pooling_prevents_capture, ragged_batch_logits)
from .MLP import require_gpu_param
from .loss import ClassificationLoss, accuracy_of, check_loss_options
from .sharding import FlatGradAllReduce
from .synthetic import GraphBatch

ALIGN = 64  # floats: every parameter starts on a 256-B boundary of the flat buffer (the MLP kernels want 16-B aligned weights)


def _layout(params, align: int = ALIGN):
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += (p.numel() + align - 1) // align * align
    return offs, off


class FlatParameters:
    """Re-homes every trainable parameter of ``module`` as a view of ONE flat fp32 buffer (``flat``) and provides the
    matching flat gradient buffer (``grad``; ``p.grad`` become views of it through ``reducer``).  Offsets are padded
    to 256 B; the gaps hold zeros in both buffers and stay zero under Adam (0 gradient -> 0 update).

    ``state_dict`` keys, shapes and values are unchanged; ``module.to(...)`` afterwards would detach the views, so
    construct this last."""

    def __init__(self, module: nn.Module, group=None, average: bool = True):
        named = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        if not self.params:
            raise ValueError("module has no trainable parameters")
        dev = require_gpu_param(self.params[0], "FlatParameters")
        if any(p.dtype != torch.float32 or p.device != dev for p in self.params):
            raise TypeError("FlatParameters: float32 parameters on one GPU expected")
        self.offsets, self.numel = _layout(self.params)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                view = self.flat[off:off + p.numel()].view_as(p)
                view.copy_(p)
                p.data = view
        self.reducer = _AlignedReducer(self.params, self.grad, self.offsets, group, average)


class _AlignedReducer(FlatGradAllReduce):
    """FlatGradAllReduce over a caller-provided flat buffer with padded offsets (always packs: the fused optimizer reads
    the flat buffer)."""

    def __init__(self, params, flat, offsets, group, average):
        self.params, self.group, self.average, self.pack_always = list(params), group, average, True
        self.flat, self.numel = flat, flat.numel()
        self.views = [flat[off:off + p.numel()].view_as(p) for p, off in zip(self.params, offsets)]
        self.collectives = 0


LR_SCHEDULE_KEYS = ("kind", "warmup_steps", "total_steps", "min_lr", "gamma", "every")
OPTIMIZERS = ("adam", "adamw", "sgd")


def lr_at(t: int, lr: float, kind: str = "constant", warmup_steps: int = 0, total_steps: int = 0, min_lr: float = 0.0,
          gamma: float = 0.1, every: int = 1) -> float:
    """Learning rate of optimizer step ``t`` (1-based), the closed form the control tick evaluates on the device
    (csrc/optimizer_ctl.hip, same operations in the same order): ``lr * (t / warmup_steps)`` up to ``warmup_steps`` (reaching ``lr``
    there), then ``constant``; ``cosine`` from ``lr`` down to ``min_lr`` at ``total_steps`` and held afterwards; or ``step``,
    ``lr * gamma ** k`` after ``k`` whole periods of ``every`` steps past the warm-up."""
    t = int(t)
    if t <= warmup_steps:
        return lr * (float(t) / float(warmup_steps))  # exactly lr at t == warmup_steps
    if kind == "cosine":
        if t >= total_steps:
            return min_lr
        progress = float(t - warmup_steps) / float(total_steps - warmup_steps)
        return min_lr + 0.5 * (lr - min_lr) * (1.0 + math.cos(math.pi * progress))
    if kind == "step":
        return lr * gamma ** float((t - warmup_steps) // every)
    if kind != "constant":
        raise ValueError(f"lr schedule kind {kind!r}: one of {sorted(native.LR_SCHEDULES)} expected")
    return lr


def check_optimizer_options(optimizer: str = "adam", lr: float = 1e-3, weight_decay: float = 0.0, momentum: float = 0.0,
                            nesterov: bool = False, max_grad_norm: float | None = None, lr_schedule: dict | None = None) -> dict:
    """ValueError for an unknown name or values that do not go together; returns the schedule as ``lr_at``'s keywords
    (``{"kind": "constant"}`` for None).  Touches no device."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer {optimizer!r}: one of {OPTIMIZERS} expected")
    finite = lambda v: isinstance(v, numbers.Real) and math.isfinite(v)  # noqa: E731  (NumPy scalars included)
    if not (finite(lr) and lr >= 0):
        raise ValueError(f"lr {lr!r}: a finite value >= 0 expected")
    if not (finite(weight_decay) and weight_decay >= 0):
        raise ValueError(f"weight_decay {weight_decay!r}: a finite value >= 0 expected")
    if not (finite(momentum) and momentum >= 0):
        raise ValueError(f"momentum {momentum!r}: a finite value >= 0 expected")
    if optimizer != "sgd" and (momentum != 0 or nesterov):
        raise ValueError(f"momentum / nesterov belong to optimizer='sgd', not {optimizer!r} (Adam's momentum is betas[0])")
    if nesterov and momentum == 0:
        raise ValueError("nesterov=True needs momentum > 0")
    if optimizer == "adamw" and lr * weight_decay >= 1:
        raise ValueError(f"adamw: lr * weight_decay = {lr * weight_decay} must stay below 1 (the decay factor 1 - lr * weight_decay)")
    if max_grad_norm is not None and not (finite(max_grad_norm) and max_grad_norm > 0):
        raise ValueError(f"max_grad_norm {max_grad_norm!r}: None or a finite value > 0 expected")
    sched = {"kind": "constant", "warmup_steps": 0, "total_steps": 0, "min_lr": 0.0, "gamma": 0.1, "every": 1}
    if lr_schedule is not None:
        if not isinstance(lr_schedule, dict):
            raise ValueError("lr_schedule: a dict expected")
        unknown = sorted(set(lr_schedule) - set(LR_SCHEDULE_KEYS))
        if unknown:
            raise ValueError(f"lr_schedule: unknown keys {unknown}; {LR_SCHEDULE_KEYS} expected")
        sched.update(lr_schedule)
    kind = sched["kind"]
    if kind not in native.LR_SCHEDULES:
        raise ValueError(f"lr schedule kind {kind!r}: one of {sorted(native.LR_SCHEDULES)} expected")
    for key in ("warmup_steps", "total_steps", "every"):
        if not isinstance(sched[key], int) or isinstance(sched[key], bool) or sched[key] < 0:
            raise ValueError(f"lr_schedule[{key!r}] = {sched[key]!r}: a count of optimizer steps (int >= 0) expected")
    if kind == "cosine":
        if sched["total_steps"] <= sched["warmup_steps"]:
            raise ValueError("cosine schedule: total_steps must exceed warmup_steps")
        if not (finite(sched["min_lr"]) and 0 <= sched["min_lr"] <= lr):
            raise ValueError(f"cosine schedule: min_lr {sched['min_lr']!r} must lie in [0, lr]")
    if kind == "step" and not (sched["every"] >= 1 and finite(sched["gamma"]) and sched["gamma"] > 0):
        raise ValueError("step schedule: every >= 1 and gamma > 0 expected")
    return sched


class _Controls:
    """Device state of a controlled step (``native.optimizer_ctl_step``, DESIGN K22): the tick's scalars, the skip counter and
    the partials of the gradient-norm pass, with the ``native.OptCtl`` that holds the run's hyper-parameters."""

    def __init__(self, device, rule: str, lr: float, schedule: dict, max_grad_norm, skip_nonfinite: bool, **hyper):
        self.schedule = schedule
        s = dict(schedule)
        self.ctl = native.opt_ctl(rule, lr, max_grad_norm=max_grad_norm, check_nonfinite=skip_nonfinite, schedule=s.pop("kind"),
                                  **s, **hyper)
        # step_size, bc2_sqrt, decay, clip_coef, lr, grad_norm: no norm taken yet (and never, without clipping or the check)
        first = [0.0, 0.0, 1.0, 1.0, lr_at(1, lr, **schedule), float("nan")]
        self.scalars = torch.tensor(first + [0.0] * (native.OPT_SCALARS - len(first)), dtype=torch.float32, device=device)
        self.skipped = torch.zeros(2, dtype=torch.int64, device=device)
        self.uses_norm = bool(self.ctl.clip or self.ctl.check_nonfinite)
        self.partials = torch.zeros(native.GRAD_NORM_BLOCKS, dtype=torch.float64, device=device) if self.uses_norm else None

    def step(self, fp: FlatParameters, state1, state2, step_count: torch.Tensor) -> None:
        native.optimizer_ctl_step(fp.flat, fp.grad, state1, state2, step_count, self.scalars, self.skipped, self.partials, self.ctl)


class _FlatOptimizer:
    """What ``FusedAdam`` and ``FusedSGD`` share: the flat buffers, the device step counter, the three device tensors a run
    reports (``grad_norm``: the norm before clipping, NaN when no norm pass runs; ``current_lr``; ``skipped_steps``), and a
    snapshot of every tensor a step writes."""

    def _init_flat(self, flat_params: FlatParameters, controls: _Controls) -> None:
        self.fp, self._controls = flat_params, controls
        self.step_count = torch.zeros(1, dtype=torch.int64, device=flat_params.flat.device)
        self.grad_norm, self.current_lr = controls.scalars[5:6], controls.scalars[4:5]
        self.skipped_steps = controls.skipped[0:1]

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.fp.reducer.zero_grad()

    def _state(self):
        raise NotImplementedError

    def state_snapshot(self):
        return [t.clone() for t in self._state()]

    def state_restore(self, snap) -> None:
        for dst, src in zip(self._state(), snap):
            dst.copy_(src)


class FusedAdam(_FlatOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) semantics (amsgrad off) as one launch over the flat
    buffers of a ``FlatParameters`` (``gnc_adam_step_f32``).  The step counter is a device tensor, so ``step()`` is
    the same launch sequence every time (hipGraph-capturable).

    With any of the keyword options the step goes through the controlled path instead (``native.optimizer_ctl_step``, DESIGN K22),
    which is capturable too - the schedule reads the device counter, so ONE captured step replays a whole schedule and a second
    capture continues it: ``decoupled_weight_decay`` (torch.optim.AdamW: ``p *= 1 - lr * weight_decay`` in place of the L2 term),
    ``max_grad_norm`` (the gradient is scaled by ``min(1, max_grad_norm / (norm + 1e-6))`` as it is read - ``fp.grad`` itself is not
    rewritten - and a step whose gradient holds a NaN or an inf is skipped and counted, where ``clip_grad_norm_`` would poison every
    parameter), ``lr_schedule`` (``lr_at``'s keywords as a dict) and ``skip_nonfinite`` (the skip without clipping)."""

    def __init__(self, flat_params: FlatParameters, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, *, decoupled_weight_decay: bool = False, max_grad_norm: float | None = None,
                 lr_schedule: dict | None = None, skip_nonfinite: bool = False):
        rule = "adamw" if decoupled_weight_decay else "adam"
        schedule = check_optimizer_options(rule, lr, weight_decay, max_grad_norm=max_grad_norm, lr_schedule=lr_schedule)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.controlled = bool(decoupled_weight_decay or max_grad_norm is not None or lr_schedule is not None or skip_nonfinite)
        dev = flat_params.flat.device
        self._init_flat(flat_params, _Controls(dev, rule, self.lr, schedule, max_grad_norm, skip_nonfinite, betas=self.betas,
                                               eps=self.eps, weight_decay=self.weight_decay))
        self.exp_avg = torch.zeros_like(flat_params.flat)
        self.exp_avg_sq = torch.zeros_like(flat_params.flat)
        self._scratch = torch.zeros(2, dtype=torch.float32, device=dev)

    def step(self, reduce: bool = True, grads=None) -> None:
        """Gradient pack (+ the one all-reduce when a process group with more than one rank is up) and the update.
        ``grads``: see FlatGradAllReduce.pack."""
        if reduce:
            self.fp.reducer(grads)
        if self.controlled:
            self._controls.step(self.fp, self.exp_avg, self.exp_avg_sq, self.step_count)
            return
        native.adam_step(self.fp.flat, self.fp.grad, self.exp_avg, self.exp_avg_sq, self.step_count, self._scratch, self.lr,
                         self.betas[0], self.betas[1], self.eps, self.weight_decay)

    def _state(self):
        plain = (self.fp.flat, self.exp_avg, self.exp_avg_sq, self.step_count)
        return plain + (self._controls.scalars, self._controls.skipped) if self.controlled else plain


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD(params, lr, momentum, nesterov=, weight_decay=) semantics (dampening 0, maximize off) - with ``momentum=0``
    the write-up's own rule ``w <- w - lr * dL/dw`` - as one controlled step over the flat buffers (``native.optimizer_ctl_step``,
    DESIGN K22).  Same interface and keyword options as ``FusedAdam``; the momentum buffer starts at zero, which gives torch's
    first-step ``buf = g``."""

    def __init__(self, flat_params: FlatParameters, lr: float, momentum: float = 0.0, nesterov: bool = False,
                 weight_decay: float = 0.0, max_grad_norm: float | None = None, lr_schedule: dict | None = None,
                 skip_nonfinite: bool = False):
        schedule = check_optimizer_options("sgd", lr, weight_decay, momentum, nesterov, max_grad_norm, lr_schedule)
        self.lr, self.momentum, self.nesterov, self.weight_decay = float(lr), float(momentum), bool(nesterov), float(weight_decay)
        self.controlled = True
        self._init_flat(flat_params, _Controls(flat_params.flat.device, "sgd", self.lr, schedule, max_grad_norm, skip_nonfinite,
                                               weight_decay=self.weight_decay, momentum=self.momentum, nesterov=self.nesterov))
        self.momentum_buffer = torch.zeros_like(flat_params.flat) if self.momentum != 0 else None

    def step(self, reduce: bool = True, grads=None) -> None:
        """Gradient pack (+ the one all-reduce of a multi-rank group; the norm is taken after it, the same on every rank) and the update."""
        if reduce:
            self.fp.reducer(grads)
        self._controls.step(self.fp, self.momentum_buffer, None, self.step_count)

    def _state(self):
        buf = (self.momentum_buffer,) if self.momentum_buffer is not None else ()
        return (self.fp.flat,) + buf + (self.step_count, self._controls.scalars, self._controls.skipped)


def make_optimizer(flat_params: FlatParameters, optimizer: str = "adam", lr: float = 1e-3, weight_decay: float = 0.0,
                   momentum: float = 0.0, nesterov: bool = False, max_grad_norm: float | None = None,
                   lr_schedule: dict | None = None, skip_nonfinite: bool = False):
    """The flat optimizer ``train()``'s keywords name: ``FusedAdam`` ("adam": L2 weight decay; "adamw": decoupled) or ``FusedSGD``."""
    check_optimizer_options(optimizer, lr, weight_decay, momentum, nesterov, max_grad_norm, lr_schedule)
    if optimizer == "sgd":
        return FusedSGD(flat_params, lr, momentum, nesterov, weight_decay, max_grad_norm, lr_schedule, skip_nonfinite)
    return FusedAdam(flat_params, lr, weight_decay=weight_decay, decoupled_weight_decay=optimizer == "adamw",
                     max_grad_norm=max_grad_norm, lr_schedule=lr_schedule, skip_nonfinite=skip_nonfinite)


def make_criterion(loss=None, class_weight=None, label_smoothing: float = 0.0, pos_weight: float | None = None, metrics: bool = False):
    """The criterion ``train()``'s keywords name: ``nn.CrossEntropyLoss()`` for ``loss=None`` (no other option may be given then), a
    ``ClassificationLoss`` for "ce" / "bce", or the ``ClassificationLoss`` instance passed in (the options then live in it;
    ``metrics`` switches its counting on).  ValueError before anything is allocated."""
    named = [name for name, given in (("class_weight", class_weight is not None), ("label_smoothing", label_smoothing != 0.0),
                                      ("pos_weight", pos_weight is not None)) if given]
    if loss is None:
        if named or metrics:
            raise ValueError(f"{named + ['metrics'] if metrics else named}: options of the device loss head; pass loss='ce' or 'bce' "
                             f"(loss=None is the reference's nn.CrossEntropyLoss())")
        return nn.CrossEntropyLoss()
    if isinstance(loss, ClassificationLoss):
        if named:
            raise ValueError(f"{named}: set these on the ClassificationLoss instance that was passed")
        loss.track_metrics = loss.track_metrics or bool(metrics)
        if loss.track_metrics and loss.num_classes is not None and loss.confusion is None:
            loss.confusion = torch.zeros(loss.num_classes, loss.num_classes, dtype=torch.int64, device=loss.status.device)
        return loss
    if not isinstance(loss, str):
        raise ValueError(f"loss {loss!r}: None, 'ce', 'bce' or a ClassificationLoss expected")
    check_loss_options(loss, class_weight, label_smoothing, pos_weight)
    return ClassificationLoss(loss, class_weight, label_smoothing, pos_weight, track_metrics=metrics)


def padded_capacity(needed: int, current: int = 0, quantum: int = 256) -> int:
    """Capacity of a padded capture for ``needed`` edges (or nodes): ``current`` while that still fits, otherwise half as
    much again as needed, rounded up to ``quantum`` - room to spare, so that a data set whose sizes vary around a typical
    value is captured once.  Never below ``needed``, monotone in ``needed``, and a fixed point for every size that
    fits: ``padded_capacity(m, padded_capacity(n)) == padded_capacity(n)`` for ``m <= padded_capacity(n)``."""
    needed, current = int(needed), int(current)
    if needed <= current:
        return current
    return (needed * 3 // 2 + quantum - 1) // quantum * quantum


def _world(group=None) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _step_loss(criterion, logits, labels, loss_sum: torch.Tensor, loss_scale: float = 1.0):
    """``(loss, accumulated)`` of one step: a ``ClassificationLoss`` takes the scale into its launch and, bound to ``loss_sum``, adds
    the loss there itself (``accumulated``); any other callable is called as it always was and the caller accumulates."""
    if isinstance(criterion, ClassificationLoss):
        return criterion(logits, labels, scale=loss_scale), criterion.accumulates_into(loss_sum)
    loss = criterion(logits, labels)
    if loss_scale != 1.0:
        loss = loss * loss_scale
    return loss, False


class _Through(nn.Module):
    """``functional_call`` target: runs ``fn(model)`` with the model's parameters swapped for the given ones."""

    def __init__(self, model: nn.Module, fn):
        super().__init__()
        self.model, self.fn = model, fn

    def forward(self):
        return self.fn(self.model)


class CapturedTrainStep(_Captured):
    """One training step (utils/train_model.py:37-42: forward, CE loss, zero_grad, backward, Adam) captured into a hipGraph and
    replayed per sample.  The loss of every replay is added to ``loss_sum`` (device float64) inside the graph.  Warm-up steps run
    before the capture; parameters, optimizer state, module buffers and the loss accumulator are restored afterwards, so
    constructing this object does not train.

    **Safe whatever the caller ran before.**  A parameter's ``AccumulateGrad`` node remembers the stream that was
    current when the node was created, and the node lives as long as ANY autograd graph that reached the parameter
    (a ``loss`` tensor the caller still holds is enough).  Had the caller trained eagerly on the legacy default
    stream, a backward inside the capture would find those nodes, and the autograd engine would make the legacy
    stream wait on an event of the capturing stream and accumulate there: a default-stream operation in the middle
    of a stream capture, which takes the HIP runtime down at ``hipStreamEndCapture`` (tools/repro_capture3.py
    reproduces it in plain PyTorch: MODE=stale_default crashes, fresh_default / stale_side / alias_default do not).
    The captured step therefore never differentiates the module's own parameter tensors: it runs the module through
    ``torch.func.functional_call`` on PRIVATE leaf aliases over the same storage (views of the flat buffer), whose
    autograd nodes are born on the warm-up / capture stream and die with each step's graph, and hands their gradients
    to the reducer's pack.  Nothing of the caller's autograd history is reachable from the capture.

    The feed decides what a call may bring (``matches``): ONE topology (``GNN.FixedGraphFeed``); with ``edge_capacity=C``, ANY edge
    list of at most C edges over the sample's node count; with ``node_capacity=M`` as well, for a ``CombinedModel`` with
    ``ragged_readout``, ANY graph of at most M nodes and C edges (``GNN.PaddedGraphFeed``; logits by ``GNN.graph_logits``; not with
    BatchNorm layers, whose statistics the dummy rows would enter).

    ``forward(model, x, pos, edge_index) -> logits`` replaces the default (a batched read-out, for instance) and receives the
    feed's buffers.  Over a padded feed it must build its topology from them in every call
    (a ``GraphTopology`` with deferred validation, never the cache), read out the first ``num_nodes`` rows only, and read
    ``valid_nodes`` itself; ``check()`` then sees the feed's flag alone.  ``loss_scale`` multiplies the loss
    (``1 / global graph count`` of a sharded batch).  With a process group of more than one rank the graph holds forward +
    backward + gradient pack, and every call issues the ONE all-reduce and the fused Adam launch directly after the replay."""

    def __init__(self, model: nn.Module, optimizer: FusedAdam, criterion, sample, label, loss_sum: torch.Tensor, *,
                 forward=None, loss_scale: float = 1.0, capture_error_mode: str = "global", edge_capacity: int | None = None,
                 node_capacity: int | None = None):
        who = "CapturedTrainStep"
        x, pos, edge_index = sample
        _no_capture_with_pooling(model, who)
        dev = require_gpu_param(next(model.parameters()), who)
        if node_capacity is not None:
            if edge_capacity is None:
                raise ValueError(f"{who}: node_capacity requires edge_capacity")
            if forward is None and not getattr(model, "ragged_readout", False):
                raise TypeError(f"{who}(node_capacity=...): a CombinedModel with ragged_readout = True (or forward=) expected")
        if edge_capacity is None:
            feed = FixedGraphFeed(x, pos, edge_index, dev)
            logits = lambda mod: (mod((feed.x, feed.pos, feed.edge_index)), None)
        else:
            if _has_batchnorm(model):  # LayerNorm is per row and unaffected
                raise NotImplementedError(f"{who}(edge_capacity=...): not with BatchNorm layers (norm_type='BatchNorm1d')")
            if forward is None and not (hasattr(model, "graph_net") and hasattr(model, "classifier")):
                raise TypeError(f"{who}(edge_capacity=...): pass forward= for a module that is not a CombinedModel")
            pooled = forward is None and bool(getattr(model, "pooled", False))
            feed = PaddedGraphFeed(x, pos, edge_index, edge_capacity, node_capacity, device=dev, who=who,
                                   min_rows=flatten_readout_rows(model, node_capacity, pooled))
            logits = lambda mod: graph_logits(mod, feed)
        if forward is not None:
            logits = lambda mod: (forward(mod, feed.x, feed.pos, feed.edge_index), None)
        self._init(model, optimizer, criterion, feed, torch.as_tensor(label).to(dev).clone(), logits, loss_sum, loss_scale,
                   capture_error_mode)

    def _init(self, model: nn.Module, optimizer: FusedAdam, criterion, feed, label: torch.Tensor, logits, loss_sum: torch.Tensor,
              loss_scale: float, capture_error_mode: str) -> None:
        """The capture itself, over ``feed``'s buffers and the ``label`` buffer: ``logits(mod) -> (logits, status)`` through private
        leaf aliases, warm-up, the recording, and the restore of everything they stepped (see the class docstring)."""
        self.feed, self.label, self.optimizer, self.loss_sum = feed, label, optimizer, loss_sum
        fp = optimizer.fp
        self.collective_outside = _world(fp.reducer.group) > 1
        through = _Through(model, logits)
        wanted = dict(zip(fp.names, range(len(fp.names))))
        alias, self._leaves = {}, [None] * len(fp.names)
        for name, p in model.named_parameters():
            leaf = p.detach()
            if name in wanted:
                leaf.requires_grad_(True)
                self._leaves[wanted[name]] = leaf
            alias["model." + name] = leaf
        if any(l is None for l in self._leaves):
            raise RuntimeError("CapturedTrainStep: the optimizer's FlatParameters were built over another module")
        leaves, outside = self._leaves, self.collective_outside

        def one_step():  # closes over no ``self``: the object that keeps it (``_record``) must not become a reference cycle
            out, status = torch.func.functional_call(through, alias, ())
            loss, accumulated = _step_loss(criterion, out, label, loss_sum, loss_scale)
            for leaf in leaves:                                                        # utils/train_model.py:40
                leaf.grad = None
            loss.backward()                                                            # :41
            grads = [leaf.grad for leaf in leaves]
            if outside:
                fp.reducer.pack(grads)
            else:
                optimizer.step(grads=grads)                                            # :42 (pack + fused Adam)
            if not accumulated:
                loss_sum.add_(loss.detach().double())
            return status

        def warm():
            one_step()
            if outside:
                self._finish()
            for leaf in leaves:  # the recording starts without gradients
                leaf.grad = None

        snap = optimizer.state_snapshot()
        tracked = criterion if isinstance(criterion, ClassificationLoss) else None  # its counts and flag must not see the warm-up
        criterion_snap = tracked.state_snapshot() if tracked is not None else None
        buffers = [(b, b.clone()) for b in model.buffers()]  # BatchNorm statistics must not absorb the warm-up either
        keep = loss_sum.clone()
        self._status = self._record(fp.flat.device, one_step, 3, warm, capture_error_mode)
        optimizer.state_restore(snap)
        if tracked is not None:
            tracked.state_restore(criterion_snap)
        with torch.no_grad():
            for b, saved in buffers:
                b.copy_(saved)
        loss_sum.copy_(keep)

    def _finish(self) -> None:
        """Multi-rank tail of a step: the ONE collective over the packed flat buffer, then the fused Adam launch."""
        self.optimizer.fp.reducer.allreduce()
        self.optimizer.step(reduce=False)

    def replay(self) -> None:
        """The step on whatever the captured input buffers hold (``self.x`` / ``self.pos`` / ``self.label``)."""
        self.graph.replay()
        if self.collective_outside:
            self._finish()

    def __call__(self, sample, label) -> None:
        self.feed(*sample)
        self.label.copy_(torch.as_tensor(label), non_blocking=True)
        self.replay()


class CapturedRaggedBatchStep(CapturedTrainStep):
    """One training step on ANY mini-batch of G graphs with at most ``node_capacity`` nodes and ``edge_capacity`` edges in all
    (superpixel batches: a new region adjacency and new node counts every batch): ``CapturedTrainStep`` over a
    ``GNN.RaggedBatchFeed``, whose one launch also carries the labels, and ``GNN.ragged_batch_logits`` - mean cross-entropy over the
    G graphs.  Slack rows ``[N, node_capacity)`` belong to no graph and the dummies only talk to dummies, so both contribute exact
    zeros to the logits and to every gradient.  G is fixed per capture; a call with a batch that does not ``matches`` raises
    ValueError.  BatchNorm layers: NotImplementedError (the dummy rows would enter the batch statistics)."""

    def __init__(self, model: nn.Module, optimizer: FusedAdam, criterion, batch: GraphBatch, labels, loss_sum: torch.Tensor, *,
                 edge_capacity: int, node_capacity: int, loss_scale: float = 1.0, capture_error_mode: str = "global"):
        who = "CapturedRaggedBatchStep"
        dev = require_gpu_param(next(model.parameters()), who)
        if not isinstance(model, CombinedModel):
            raise TypeError(f"{who}: a CombinedModel expected")
        _no_capture_with_pooling(model, who)
        if _has_batchnorm(model):
            raise NotImplementedError(f"{who}: not with BatchNorm layers (norm_type='BatchNorm1d')")
        feed = RaggedBatchFeed(batch, edge_capacity, node_capacity, dev, with_labels=True, who=who)
        feed(batch, labels)
        self._init(model, optimizer, criterion, feed, feed.labels, lambda mod: ragged_batch_logits(mod, feed), loss_sum, loss_scale,
                   capture_error_mode)

    def __call__(self, batch, labels) -> None:
        self.feed(batch, labels)
        self.replay()


class _TensorFeed:
    """ONE input buffer of the sample's shape and dtype; a call is one copy."""

    edge_capacity = node_capacity = pos = edge_index = None

    def __init__(self, sample: torch.Tensor, device):
        self.x = sample.to(device).clone()

    def __call__(self, sample: torch.Tensor) -> None:
        self.x.copy_(sample, non_blocking=True)

    def check(self, status) -> None:
        pass


class CapturedTensorStep(CapturedTrainStep):
    """One training step on a plain tensor batch (the reference's image-MLP path, main.py:21-29: ``mod(x)`` on float32
    ``[B, 3, R, R]``, mean cross-entropy over the B labels): ``CapturedTrainStep`` over a ``_TensorFeed``.  Everything runs on a
    single stream.  ``matches(sample, label)``: same shapes and dtype (a short last batch does not match and runs eagerly)."""

    def __init__(self, model: nn.Module, optimizer: FusedAdam, criterion, sample: torch.Tensor, label, loss_sum: torch.Tensor, *,
                 loss_scale: float = 1.0, capture_error_mode: str = "global"):
        dev = require_gpu_param(next(model.parameters()), "CapturedTensorStep")
        feed = _TensorFeed(sample, dev)
        self._init(model, optimizer, criterion, feed, torch.as_tensor(label).to(dev).clone(), lambda mod: (mod(feed.x), None),
                   loss_sum, loss_scale, capture_error_mode)

    def matches(self, sample, label=None) -> bool:
        return (isinstance(sample, torch.Tensor) and sample.shape == self.x.shape and sample.dtype == self.x.dtype
                and (label is None or torch.as_tensor(label).shape == self.label.shape))

    def __call__(self, sample, label) -> None:
        self.feed(sample)
        self.label.copy_(torch.as_tensor(label), non_blocking=True)
        self.replay()


# --------------------------------------------------------------------------- the run's side effects
class RunJournal:
    """Everything the reference's train() writes or prints besides checkpoints: the timestamped
    ``training_logs_<stamp>.txt`` (header :26-30, two lines per epoch :52-54, footer :76-80) and the console lines
    (:19, :48, :50, :63, :68, :74).  The line formats are contract (golden G8 compares them)."""

    RULE = "-" * 50

    def __init__(self, directory: str, epochs: int, patience: int):
        os.makedirs(directory, exist_ok=True)
        print(f"Training model in {directory}")
        opened = datetime.now()
        self.epochs = epochs
        self.path = os.path.join(directory, f"training_logs_{opened.strftime('%Y%m%d_%H%M%S')}.txt")
        self._append([f"Training started at: {opened.strftime('%Y-%m-%d %H:%M:%S')}", f"Epochs: {epochs}, Patience: {patience}",
                      f"Output path: {directory}", self.RULE], mode="w")

    def _append(self, lines, mode: str = "a") -> None:
        with open(self.path, mode) as f:
            f.write("".join(line + "\n" for line in lines))

    def epoch(self, number: int, avg_loss: float, seconds: float, accuracy: float | None = None) -> None:
        """``accuracy``: the epoch's training accuracy, added to the loss line when the run tracks metrics (not in the reference)."""
        tag = f"Epoch {number}/{self.epochs}"
        line = f"{tag}, avg_loss={avg_loss:.4f}" + (f", accuracy={accuracy:.4f}" if accuracy is not None else "")
        print(line)
        print(f"epoch: {number} needed {seconds} time")
        self._append([line, f"{tag}, needed {seconds / 60:.2f} minutes"])

    def saved(self, kind: str, path: str) -> None:
        print(f"Saved {kind} model: {path}")

    def stopped_early(self, number: int) -> None:
        print(f"Early stopping at epoch {number}")

    def close(self, best_loss: float, final_path: str) -> None:
        self._append([self.RULE, f"Training completed at: {datetime.now().strftime('%Y-%m-%d %H:%M:%S')}",
                      f"Best loss achieved: {best_loss:.4f}", f"Final model saved: {final_path}"])


class PlateauStopper:
    """Early stopping on the average TRAINING loss (utils/train_model.py:57-69): an epoch either sets a new best (strictly
    lower) or counts as stale; ``patience`` stale epochs in a row end the run."""

    def __init__(self, patience: int):
        self.patience, self.best, self.stale = patience, float("inf"), 0

    def observe(self, value: float) -> bool:
        """True when ``value`` is a new best."""
        if value < self.best:
            self.best, self.stale = value, 0
            return True
        self.stale += 1
        return False

    @property
    def exhausted(self) -> bool:
        return self.stale >= self.patience


class CheckpointShelf:
    """The ``.pth`` files of a run (:61-62, :72-73): state dicts under the reference's keys, CPU tensors."""

    def __init__(self, model: nn.Module, directory: str):
        self.model, self.directory = model, directory

    def _write(self, filename: str) -> str:
        path = os.path.join(self.directory, filename)
        torch.save({k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}, path)
        return path

    def best(self, epoch_number: int) -> str:
        return self._write(f"best_model_epoch{epoch_number}.pth")

    def final(self) -> str:
        return self._write("final_model.pth")


def _batched_forward(model, batch: GraphBatch, dev):
    """``forward(mod, x, pos, edge_index) -> logits [G, C]`` of a mini-batch, for the eager step, a capture's ``forward=`` and the
    scorers alike: the ``num_graphs`` form for graphs of exactly ``num_nodes`` nodes on a model without ``ragged_readout`` and
    without top-K pooling (behind it the flatten read-out needs the offsets), else the ``graph_ptr`` form (a device copy made
    here, once)."""
    sizes = batch.graph_ptr[1:] - batch.graph_ptr[:-1]
    pooling = bool(getattr(getattr(model, "graph_net", None), "pooling", False))
    if not getattr(model, "ragged_readout", False) and not pooling and bool((sizes == model.num_nodes).all()):
        G = batch.num_graphs
        return lambda mod, xx, pp, ee: mod.forward_batched(xx, pp, ee, num_graphs=G)
    gptr = batch.graph_ptr.to(dev)
    return lambda mod, xx, pp, ee: mod.forward_batched(xx, pp, ee, graph_ptr=gptr)


def _forward_of(model, sample, dev):
    """The model's output for one loader item, inputs moved to ``dev``: a ``GraphBatch`` through ``forward_batched``, an
    ``(x, pos, edge_index)`` graph or a plain tensor through ``model(sample)``."""
    if isinstance(sample, GraphBatch):
        x, pos = sample.x.to(dev, non_blocking=True), sample.pos.to(dev, non_blocking=True)
        return _batched_forward(model, sample, dev)(model, x, pos, sample.edge_index)
    if isinstance(sample, (tuple, list)) and len(sample) == 3:
        # edge_index stays where it is: a host tensor is looked up in the topology cache by content, so equal
        # topologies are sorted once, not once per sample
        return model((sample[0].to(dev, non_blocking=True), sample[1].to(dev, non_blocking=True), sample[2]))
    return model(sample.to(dev, non_blocking=True))


def _repeats(previous, parts) -> bool:
    """``parts`` = ``(x, pos, edge_index, graph_ptr or None)`` of a sample with the shapes, the graph offsets and the topology of
    ``previous``: what ONE fixed-topology capture serves."""
    return (previous[0].shape == parts[0].shape and previous[1].shape == parts[1].shape
            and (parts[3] is None or torch.equal(previous[3], parts[3])) and _same_topology(previous[2], parts[2]))


def _kind_and_size(parts):
    """``((graph count, feature widths), nodes, edges)`` of a sample's parts."""
    x, pos, edge_index, graph_ptr = parts
    graphs = 1 if graph_ptr is None else graph_ptr.numel() - 1
    return (graphs, tuple(x.shape[1:]), tuple(pos.shape[1:])), int(x.size(0)), int(edge_index.size(1))


class _SampleKind(NamedTuple):
    """What ``_PaddedCaptures`` is told about the samples it serves."""
    parts: Callable    # sample -> (x, pos, edge_index, graph_ptr or None): its kind, node count and edge count are read there
    allowed: bool      # this model's step can run over padded buffers
    nodes_vary: bool   # a sample may have another node count than the one before it
    node_form: bool    # ... and the first capture has node slots to spare already (else the edge-only form, until a count differs)
    repeats: bool      # a sample that repeats the eager one before it is eligible too (else it is a fixed-topology capture's case)


def _batches(model) -> _SampleKind:
    return _SampleKind(lambda b: (b.x, b.pos, b.edge_index, b.graph_ptr), isinstance(model, CombinedModel) and not _has_batchnorm(model),
                       True, True, False)


def _single_graphs(model) -> _SampleKind:  # the stepper tries the fixed-topology capture before it asks
    return _SampleKind(lambda s: (*s, None), hasattr(model, "graph_net") and hasattr(model, "classifier") and not _has_batchnorm(model),
                       bool(getattr(model, "ragged_readout", False)), False, True)


class _PaddedCaptures:
    """THE rule for serving a stream of new topologies from one padded capture that only grows - single graphs and mini-batches in
    the training loop, mini-batches in ``evaluate`` / ``predict``, each with an instance (and so a capture count) of its own:
    ``get(sample, previous)`` returns the capture object that serves ``sample``, or None for a sample that runs eagerly.

    The capture that matches is returned.  Otherwise a capture is made for an eligible sample only: on an ``allowed`` model, one
    of the kind (graph count, at most ``native.PAD_BATCH_MAX_GRAPHS``, and feature widths) of the eager sample before it or of
    the capture it outgrew.  Capacities come from ``padded_capacity`` (edges in steps of 256, nodes in steps of 32): the first
    capture is sized from the larger of the two samples, a later one from the sample that outgrew the capture, and no capacity
    ever shrinks.  The capture that is replaced is checked first (``check()``: its flags would be lost with it); at most ``limit``
    captures are made, after which the capture stays for every sample that fits and an oversize sample runs eagerly on its own,
    as a sample of another kind does (a short last batch).  In the edge-only form (``node_capacity=None``) another node count is
    ineligible, or - where ``nodes_vary`` - turns every later capture to the node-capacity form, with room for the node count
    that the edge-only captures served."""

    def __init__(self, model, make, limit: int, kind=_batches):
        self.make, self.limit = make, limit  # make(sample, *args, edge_capacity=, node_capacity=) -> the capture object
        self.parts, self.allowed, self.nodes_vary, self.node_form, self.repeats = kind(model)
        self.current = None
        self.captures = 0
        self.edge_capacity = self.node_capacity = 0
        self._kind, self._nodes = None, 0  # of the samples the current capture was made for; the largest node count among them

    def get(self, sample, previous, *args):
        """``previous``: the parts ``(x, pos, edge_index, graph_ptr or None)`` of the last sample that ran eagerly, or None;
        ``args`` go to ``make`` behind the sample (the labels of a training step)."""
        cur = self.current
        if cur is not None and cur.matches(sample):
            return cur
        if not self.allowed or self.captures >= self.limit:
            return None
        parts = self.parts(sample)
        kind, nodes, edges = _kind_and_size(parts)
        if cur is not None:  # outgrown, if it is of the capture's kind
            known, seen_nodes, seen_edges = self._kind, self._nodes, 0
        elif previous is not None and (self.repeats or not _repeats(previous, parts)):
            known, seen_nodes, seen_edges = _kind_and_size(previous)
        else:
            return None
        node_form = self.node_form or (self.nodes_vary and nodes != seen_nodes)
        if kind != known or kind[0] > native.PAD_BATCH_MAX_GRAPHS or not (node_form or nodes == seen_nodes):
            return None
        if cur is not None:
            cur.check()
        self._kind, self._nodes, self.node_form = kind, max(nodes, seen_nodes), node_form
        self.edge_capacity = padded_capacity(max(edges, seen_edges), self.edge_capacity)
        if node_form:
            self.node_capacity = padded_capacity(self._nodes, self.node_capacity, 32)
        self.current = self.make(sample, *args, edge_capacity=self.edge_capacity, node_capacity=self.node_capacity if node_form else None)
        self.captures += 1
        return self.current

    def check(self) -> None:
        if self.current is not None:
            self.current.check()


class _SampleStepper:
    """Runs one optimizer step per sample: the replay of a captured step where one serves the sample, the eager step otherwise.
    A sample that repeats the eager one before it gets the ONE capture of its topology (single graph, mini-batch) or shape
    (tensor batch), replayed while samples match it; every other graph or mini-batch is served under ``_PaddedCaptures``."""

    MAX_PADDED_CAPTURES = 4  # a dataset whose sizes keep outgrowing the capacity runs its oversize samples eagerly

    def __init__(self, model, optimizer, criterion, loss_sum, device, capture: bool):
        self.model, self.optimizer, self.criterion, self.loss_sum, self.device = model, optimizer, criterion, loss_sum, device
        self.capture = capture
        self.capture_ragged_batches = capture  # ragged mini-batches (superpixel graphs): CapturedRaggedBatchStep
        self.batched = False
        # one topology / one shape each: single graphs, mini-batches, plain tensor batches (the image-MLP baseline)
        self.captured = self.captured_batch = self.captured_tensor = None
        self._previous = self._previous_batch = self._previous_tensor = None  # of the last sample of the kind that ran eagerly
        self.padded = _PaddedCaptures(  # single graphs with a new topology each (superpixel graphs)
            model, lambda sample, label, **capacities: CapturedTrainStep(model, optimizer, criterion, sample, label, loss_sum,
                                                                         **capacities),
            self.MAX_PADDED_CAPTURES, _single_graphs)
        self.ragged = _PaddedCaptures(  # mini-batches of them
            model, lambda batch, labels, **capacities: CapturedRaggedBatchStep(model, optimizer, criterion, batch, labels, loss_sum,
                                                                               **capacities),
            self.MAX_PADDED_CAPTURES)

    def _replay_graph(self, sample, label) -> bool:
        """A single graph: the fixed-topology capture first, so topologies that repeat keep their own capture."""
        parts = (*sample, None)
        if self.captured is None and self._previous is not None and _repeats(self._previous, parts):
            self.captured = CapturedTrainStep(self.model, self.optimizer, self.criterion, sample, label, self.loss_sum)
        fixed = self.captured is not None and self.captured.matches(sample)
        step = self.captured if fixed else self.padded.get(sample, self._previous, label)
        if step is None:
            self._previous = parts
            return False
        step(sample, label)
        return True

    def _replay_batch(self, batch, labels) -> bool:
        """A mini-batch (mean cross-entropy over the batch): the fixed-topology capture when it has the topology of the batch
        before it (pixel / patch graphs of one size: every full batch), else the ragged-batch capture (superpixel graphs)."""
        sample = (batch.x, batch.pos, batch.edge_index)
        parts = sample + (batch.graph_ptr,)
        if self.captured_batch is None and self._previous_batch is not None and _repeats(self._previous_batch, parts):
            self.captured_batch = CapturedTrainStep(self.model, self.optimizer, self.criterion, sample, labels, self.loss_sum,
                                                    forward=_batched_forward(self.model, batch, self.device))
            self._captured_graph_ptr = batch.graph_ptr.clone()
        if (self.captured_batch is not None and torch.equal(self._captured_graph_ptr, batch.graph_ptr)
                and self.captured_batch.matches(sample)):
            self.captured_batch(sample, labels)
            return True
        step = self.ragged.get(batch, self._previous_batch, labels) if self.capture_ragged_batches else None
        if step is None:
            self._previous_batch = parts
            return False
        step(batch, labels)
        return True

    def _replay_tensor(self, sample: torch.Tensor, label) -> bool:
        """A plain tensor sample: captured once two consecutive samples share shape and dtype (and label shape), replayed while
        they keep doing so; anything else (the first sample, a short last batch) is left to the eager step.  Only this package's
        ``MLP`` is captured: its forward is a function of the input buffer and the parameters alone, on the device, which is what
        a replay repeats - an arbitrary module may read host state or copy from the host in its forward and keeps the eager step."""
        from .MLP import MLP
        if not isinstance(self.model, MLP):
            return False
        key = (sample.shape, sample.dtype, torch.as_tensor(label).shape)
        if self.captured_tensor is None and key == self._previous_tensor:
            self.captured_tensor = CapturedTensorStep(self.model, self.optimizer, self.criterion, sample, label, self.loss_sum)
        if self.captured_tensor is not None and self.captured_tensor.matches(sample, label):
            self.captured_tensor(sample, label)
            return True
        self._previous_tensor = key
        return False

    def check(self) -> None:
        self.padded.check()
        self.ragged.check()

    def __call__(self, sample, label) -> None:
        if isinstance(sample, GraphBatch):
            self.batched = True
            replay = self._replay_batch
        elif isinstance(sample, (tuple, list)) and len(sample) == 3:
            replay = self._replay_graph
        else:
            replay = self._replay_tensor if isinstance(sample, torch.Tensor) else None
        if self.capture and replay is not None and replay(sample, label):
            return
        logits = _forward_of(self.model, sample, self.device)                                  # utils/train_model.py:37
        loss, accumulated = _step_loss(self.criterion, logits, torch.as_tensor(label).to(self.device, non_blocking=True),
                                       self.loss_sum)                                          # :38
        self.optimizer.zero_grad()                                                             # :40
        loss.backward()                                                                        # :41
        self.optimizer.step()                                                                  # :42
        if not accumulated:
            self.loss_sum += loss.detach().double()                                            # :44, without the per-sample sync


def train(model, dataset, epochs, patience=5, output_path='weights', start_weights=None, *, capture: bool = True, lr: float = 1e-3,
          capture_ragged_batches: bool = False, optimizer: str = "adam", weight_decay: float = 0.0, momentum: float = 0.0,
          nesterov: bool = False, max_grad_norm: float | None = None, lr_schedule: dict | None = None,
          skip_nonfinite: bool = False, loss=None, class_weight=None, label_smoothing: float = 0.0, pos_weight: float | None = None,
          metrics: bool = False):
    """utils/train_model.py:8-81 (same positional arguments, files and log lines).  Returns a dict with the per-epoch
    average losses (the reference returns None; nothing in it reads the return value).

    Mini-batches: a ``dataset`` that yields ``(synthetic.GraphBatch, labels [B])`` - ``GraphImageFolder.loader(batch_size=B)`` -
    takes one optimizer step per batch through ``model.forward_batched`` (``_batched_forward`` picks the form); the loss is
    ``CrossEntropyLoss()``'s mean over the batch (:38 on a batched input, as the reference's image-MLP path with
    ``batch_size=8``, main.py:13-29) and the epoch average is taken over steps (:47).  ``"batched"`` in the returned dict says
    which form ran.

    Captures (``capture=True``): a single graph or a full mini-batch with the topology of the sample before it gets the ONE
    capture of that topology (``"captured"`` in the returned dict; pixel / patch graphs of one size).  Samples that bring a new
    topology each (superpixel graphs) are served from a padded capture under ``_PaddedCaptures``' rule, stated there: single
    graphs (``"captured_any_topology"``; with a node capacity, for a ``ragged_readout`` model whose node counts vary,
    ``"captured_ragged"``) and, with ``capture_ragged_batches=True`` only, mini-batches of one graph count
    (``CapturedRaggedBatchStep``: ONE feed launch and the replay per batch; ``"captured_ragged_batch"``) - the eager ragged-batch
    step has not been timed against it on an MI355X yet (``tools/latency_ragged_batch.py`` does that), and the default follows
    the measurement.  A short last batch always runs eagerly.

    Training controls (DESIGN K22; all of them run inside a captured step, none reads the device back): ``optimizer`` "adam" (the
    reference's, ``weight_decay`` as Adam's L2 term), "adamw" (decoupled decay) or "sgd" (``momentum``, ``nesterov``; the write-up's
    update rule with neither); ``max_grad_norm`` clips the gradient's global norm; ``lr_schedule`` is a dict of ``lr_at``'s keywords
    (``kind`` "constant" / "cosine" / "step", ``warmup_steps``, ``total_steps``, ``min_lr``, ``gamma``, ``every`` - counts in
    optimizer steps); ``skip_nonfinite`` (implied by clipping) drops and counts a step whose gradient holds a NaN or an inf.
    Unknown names and values that do not go together raise ValueError before anything is allocated.  The returned dict holds
    per-epoch lists ``"lr"`` and ``"grad_norm"`` (of the epoch's last step; the norm before clipping, NaN when none is taken) and
    the run's ``"skipped_steps"``, read with the epoch's loss.

    Loss (DESIGN K23): ``loss=None`` is the reference's ``nn.CrossEntropyLoss()`` on PyTorch's own ops, launch for launch as before.
    ``loss="ce"`` / ``"bce"`` - or a ``loss.ClassificationLoss`` instance - selects the device loss head, ONE launch per step for loss,
    gradient and the epoch's loss accumulator: ``class_weight`` (one weight per class) and ``label_smoothing`` for "ce";
    ``pos_weight`` and ``label_smoothing`` for "bce", the write-up's binary cross-entropy on a model with ONE logit
    (``CombinedModel(classes=1)``), labels 0 / 1.  ``metrics=True`` counts every training sample into a confusion matrix inside that
    launch: the returned dict gains per-epoch ``"accuracy"`` and ``"confusion"`` (int64 [K, K] tensors, rows = true class), read
    with the epoch's one host read and reset per epoch, and the log line gains the accuracy.  A label outside the classes raises
    IndexError at the end of its epoch.  Any of these options with ``loss=None`` is a ValueError."""
    check_optimizer_options(optimizer, lr, weight_decay, momentum, nesterov, max_grad_norm, lr_schedule)
    criterion = make_criterion(loss, class_weight, label_smoothing, pos_weight, metrics)          # :10
    if start_weights:
        model.load_state_dict(torch.load(start_weights, map_location="cpu"))           # :14-15
    dev = require_gpu_param(next(model.parameters()), "train")
    optimizer = make_optimizer(FlatParameters(model), optimizer, lr, weight_decay, momentum, nesterov, max_grad_norm, lr_schedule,
                               skip_nonfinite)                                         # :9
    journal = RunJournal(output_path, epochs, patience)
    shelf = CheckpointShelf(model, output_path)
    stopper = PlateauStopper(patience)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    head = criterion if isinstance(criterion, ClassificationLoss) else None
    if head is not None:
        head.bind_loss_sum(loss_sum)
    # this loop steps one rank's model on its own samples: with a multi-rank process group up, a captured step would
    # record (or, under gloo, host-stage) a collective per sample that nothing here asked for
    # (a model whose top-K pooling reads sizes back in its forward: no capture can record it, every step runs eagerly; padded
    # pooling layers under a pooled read-out are captured like an un-pooled model)
    stepper = _SampleStepper(model, optimizer, criterion, loss_sum, dev, capture and _world() == 1 and not pooling_prevents_capture(model))
    stepper.capture_ragged_batches = stepper.capture and capture_ragged_batches
    history, lr_history, norm_history, skipped_steps = [], [], [], 0
    accuracy_history, confusion_history = [], []
    # Belt and braces: the loop runs on a side stream, so that the eager steps in front of a capture never touch the
    # legacy default stream.  The capture itself no longer depends on it (CapturedTrainStep differentiates private
    # aliases of the parameters, see its docstring for the hipStreamEndCapture crash this used to be the only guard of).
    run_stream = torch.cuda.Stream(device=dev)
    run_stream.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(run_stream):
            for epoch in range(1, epochs + 1):
                started = time.time()
                loss_sum.zero_()
                if head is not None:
                    head.reset_metrics()
                steps = 0
                for sample, label in dataset:                                          # :35
                    stepper(sample, label)
                    steps += 1
                accuracy = None
                if head is not None and head.status is not None:  # the loss, the label flag and the counts in ONE host read
                    parts = [loss_sum.reshape(1), head.status.double()] + ([head.confusion.reshape(-1).double()] if metrics else [])
                    stats = torch.cat(parts).cpu()
                    avg_loss = float(stats[0]) / max(1, steps)
                    if int(stats[1]) & 1:
                        head.check()  # raises IndexError (and clears the flag)
                    if metrics:
                        K = head.num_classes
                        confusion_history.append(stats[2:].round().to(torch.int64).view(K, K))
                        accuracy = accuracy_of(confusion_history[-1])
                        accuracy_history.append(accuracy)
                else:
                    avg_loss = float(loss_sum.item()) / max(1, steps)                  # :47 (the epoch's one host sync)
                stepper.check()  # replayed topology builds: node ids outside the graph raise here (models/GNN.py:18-20)
                history.append(avg_loss)
                lr_history.append(float(optimizer.current_lr.item()))                 # of the epoch's last step; the stream is idle
                norm_history.append(float(optimizer.grad_norm.item()))
                skipped_steps = int(optimizer.skipped_steps.item())
                journal.epoch(epoch, avg_loss, time.time() - started, accuracy)
                if stopper.observe(avg_loss):                                          # :57-66
                    journal.saved("best", shelf.best(epoch))
                if stopper.exhausted:                                                  # :67-69
                    journal.stopped_early(epoch)
                    break
            final_path = shelf.final()                                                 # :72-74
            journal.saved("final", final_path)
            journal.close(stopper.best, final_path)
    finally:
        torch.cuda.current_stream(dev).wait_stream(run_stream)
    extra = {"accuracy": accuracy_history, "confusion": confusion_history} if metrics else {}
    return {**extra, "avg_loss": history, "best_loss": stopper.best, "log_path": journal.path,
            "lr": lr_history, "grad_norm": norm_history, "skipped_steps": skipped_steps,
            "captured": stepper.captured is not None or stepper.captured_batch is not None, "batched": stepper.batched,
            "captured_any_topology": stepper.padded.current is not None,
            "captured_ragged": stepper.padded.current is not None and stepper.padded.current.node_capacity is not None,
            "captured_ragged_batch": stepper.ragged.current is not None,
            "captured_tensor": stepper.captured_tensor is not None,
            "optimizer": optimizer}


# --------------------------------------------------------------------------- evaluation
class _BatchScorer:
    """Logits of loader items for ``evaluate`` / ``predict``: ragged mini-batches replay a ``CapturedRaggedBatchForward`` under
    the rule of the training loop (``_PaddedCaptures``); same-topology batches and single graphs (one row) run eagerly."""

    def __init__(self, model, dev, capture: bool):
        # pooling that reads sizes back: eager (no capture)
        self.model, self.dev, self.capture = model, dev, capture and not pooling_prevents_capture(model)
        self.ragged = _PaddedCaptures(
            model, lambda batch, **capacities: CapturedRaggedBatchForward(model, batch, **capacities),
            _SampleStepper.MAX_PADDED_CAPTURES)
        self._previous = None

    def __call__(self, sample):
        if self.capture and isinstance(sample, GraphBatch):
            forward = self.ragged.get(sample, self._previous)
            if forward is not None:
                return forward(sample).clone()  # the capture's output buffer is rewritten by the next replay
            self._previous = (sample.x, sample.pos, sample.edge_index, sample.graph_ptr)
        logits = _forward_of(self.model, sample, self.dev)
        return logits.unsqueeze(0) if logits.dim() == 1 else logits

    def check(self) -> None:
        self.ragged.check()


def predict(model, loader, *, capture: bool = True, binary: bool = False):
    """``(logits [n, C], probabilities [n, C])`` of every sample of ``loader`` in loader order, on the model's device - the pair
    ``utils/inference.py:68-71`` returns per image (softmax over the classes).  ``loader`` yields ``(sample, label)`` with a
    single graph or a ``GraphBatch`` (``GraphImageFolder.loader(shuffle=False, batch_size=...)``); labels are not read.
    ``capture``: ragged mini-batches (superpixel graphs) replay a captured forward (``_BatchScorer``); an edge list that leaves
    its graph raises IndexError at the end.  ``binary``: the model has ONE logit z per sample (trained with ``loss="bce"``) and the
    probabilities are ``[1 - sigmoid(z), sigmoid(z)]``, shape [n, 2]."""
    dev = require_gpu_param(next(model.parameters()), "predict")
    with torch.no_grad():
        score = _BatchScorer(model, dev, capture)
        rows = [score(sample) for sample, _ in loader]
        if not rows:
            raise ValueError("predict: the loader yielded nothing")
        logits = torch.cat(rows)
        score.check()
        if binary:
            if logits.size(1) != 1:
                raise ValueError(f"predict(binary=True): a model with ONE logit per sample expected, got {logits.size(1)}")
            return logits, torch.cat([torch.sigmoid(-logits), torch.sigmoid(logits)], dim=1)
        return logits, torch.softmax(logits, dim=-1)


def _evaluate_with_head(model, loader, capture: bool, criterion: ClassificationLoss, dev):
    """``evaluate`` on the device loss head: per batch ONE launch in scoring mode adds the batch's summed loss to a float64
    accumulator and its counts to a confusion matrix; one host read at the end."""
    head = ClassificationLoss(criterion.kind, criterion._class_weight, criterion.label_smoothing,
                              criterion.pos_weight if criterion.kind == "bce" else None, reduction="sum", track_metrics=True)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
    head.bind_loss_sum(loss_sum)
    count = 0
    with torch.no_grad():
        score = _BatchScorer(model, dev, capture)
        for sample, label in loader:
            labels = torch.as_tensor(label).to(dev, non_blocking=True).reshape(-1)
            head(score(sample), labels)
            count += int(labels.numel())
        if head.confusion is None:
            raise ValueError("evaluate: the loader yielded nothing")
        stats = torch.cat([loss_sum, head.status.double(), head.confusion.reshape(-1).double()]).cpu()  # the one host read
        score.check()
    if int(stats[1]) & 1:
        raise IndexError(f"evaluate: a label lies outside the {head.num_classes} classes [0, {head.num_classes})")
    confusion = stats[2:].round().to(torch.int64).view(head.num_classes, head.num_classes)
    return {"loss": float(stats[0]) / count, "accuracy": float(confusion.diagonal().sum()) / count, "confusion": confusion,
            "count": count}


def evaluate(model, loader, *, capture: bool = True, criterion=None):
    """Scores ``model`` on every sample of ``loader`` (either loader form) under ``no_grad``: ``{"loss": mean cross-entropy over
    the samples, "accuracy", "confusion": int64 [C, C] with rows = true class and columns = predicted class, "count"}``.
    Loss and confusion matrix are accumulated on the device (integer scatter-adds, float64 loss) and read ONCE at the end.
    ``capture``: ragged mini-batches (superpixel graphs) replay a captured forward (``_BatchScorer``); an edge list that leaves
    its graph raises IndexError at the end.  ``criterion``: a ``loss.ClassificationLoss`` - loss and counts then come from ONE launch of
    the device loss head per batch (scoring mode), with ITS definition of the loss (kind, class weights, smoothing, pos_weight), summed
    over the samples and divided by their number; the criterion's own counts and accumulator are not touched."""
    dev = require_gpu_param(next(model.parameters()), "evaluate")
    if criterion is not None:
        if not isinstance(criterion, ClassificationLoss):
            raise TypeError("evaluate(criterion=...): a ClassificationLoss (or None) expected")
        return _evaluate_with_head(model, loader, capture, criterion, dev)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
    confusion, count = None, 0
    with torch.no_grad():
        score = _BatchScorer(model, dev, capture)
        for sample, label in loader:
            logits = score(sample)
            labels = torch.as_tensor(label).to(dev, non_blocking=True).reshape(-1)
            if confusion is None:
                classes = logits.size(1)
                confusion = torch.zeros(classes * classes, dtype=torch.int64, device=dev)
            loss_sum += nn.functional.cross_entropy(logits, labels, reduction="sum").double()
            confusion.index_add_(0, labels * classes + logits.argmax(dim=1), torch.ones_like(labels))
            count += int(labels.numel())
        if confusion is None:
            raise ValueError("evaluate: the loader yielded nothing")
        stats = torch.cat([loss_sum, confusion.double()]).cpu()  # the one host read
        score.check()
    confusion = stats[1:].round().to(torch.int64).view(classes, classes)
    return {"loss": float(stats[0]) / count, "accuracy": float(confusion.diagonal().sum()) / count, "confusion": confusion,
            "count": count}
