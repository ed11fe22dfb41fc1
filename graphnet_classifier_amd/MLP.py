"""Drop-in for the reference's ``models/MLP.py``: same constructor, same ``state_dict``
keys (``model.<i>.weight`` ...), forward executed by the fused HIP kernel K4 (``norm_type='BatchNorm1d'``: K4 + the batch-norm
kernels K14).

Reference: models/MLP.py:5-47.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as Fn
from . import native


def default_device() -> torch.device:
    """Device new modules are created on: the current ROCm device when one is visible (the
    reference never calls ``.to(device)``, so a drop-in has to place itself), else CPU -- on
    which only construction and state-dict handling work, never ``forward``."""
    if torch.cuda.is_available():
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


def require_gpu_param(p: Tensor, what: str) -> torch.device:
    if not p.is_cuda:
        raise RuntimeError(
            f"{what}: parameters are on {p.device}; the forward path exists only as HIP kernels for the MI355X "
            f"(no CPU fallback).  Construct the module on a machine with a visible GPU or call .to('cuda').")
    return p.device


class MLP(nn.Module):
    def __init__(
        self,
        in_dim: int,
        out_dim: int,
        hidden_dim: int = 128,
        hidden_layers: int = 2,
        activation: str = "ReLU",
        initializer: None | str = None,
        norm_type: None | str = "LayerNorm",
    ):
        """Linear/act x hidden_layers, Linear, optional norm (models/MLP.py:24-37).

        The Sequential built here has exactly the reference's module order (Linear at even positions,
        the shared activation module between them, the norm last) so ``state_dict`` keys and the random
        initialisation under a given seed are the same."""
        super().__init__()
        self.activation_name = activation
        self.activation = getattr(nn, activation)()  # AttributeError for an unknown name, as in the reference
        if norm_type is not None:
            assert norm_type in ["LayerNorm", "BatchNorm1d"]  # models/MLP.py:30-33
        self.norm_type = norm_type
        widths = [in_dim] + [hidden_dim] * max(int(hidden_layers), 1) + [out_dim]
        chain = []
        for k in range(len(widths) - 1):
            chain.append(nn.Linear(widths[k], widths[k + 1]))
            if k + 2 < len(widths):
                chain.append(self.activation)
        if norm_type is not None:
            chain.append(getattr(nn, norm_type)(out_dim))
        self.model = nn.Sequential(*chain)
        if initializer is not None:
            self.initializer = getattr(nn.init, initializer)
            for tensor in self.model.parameters():
                if tensor.requires_grad and tensor.dim() > 1:
                    self.initializer(tensor)
        self.to(default_device())

    # -- pieces of the Sequential the kernel consumes ------------------------------------
    def _linears(self):
        return [m for m in self.model if isinstance(m, nn.Linear)]

    def _kernel_params(self):
        """``(weights, biases, ln)`` as the kernels take them: one entry per Linear, ``ln = (gamma, beta, eps)`` behind a
        LayerNorm and None otherwise."""
        lin, norm = self._linears(), self.model[-1]
        ln = (norm.weight, norm.bias, norm.eps) if isinstance(norm, nn.LayerNorm) else None
        return [m.weight for m in lin], [m.bias for m in lin], ln

    def _act_param(self) -> float:
        a = self.activation
        return float(getattr(a, "negative_slope", getattr(a, "alpha", 0.0)))

    def _batchnorm_in_library(self, norm) -> bool:
        """Is this BatchNorm1d served by the K14 kernels?  The constructor defaults are (``momentum=None`` would need a host-side
        running average factor); any other configuration stays on the PyTorch-ROCm module."""
        return bool(norm.affine and norm.track_running_stats and norm.momentum == 0.1 and norm.running_mean is not None
                    and norm.weight.is_cuda and norm.weight.dtype == torch.float32 and norm.num_features <= native.BN_MAX_WIDTH)

    def _folded_batchnorm(self, weights, biases, norm):
        """(weights, biases) of the Linear chain with the eval-mode BatchNorm folded into the last Linear (K14 fold kernel).
        Formed from the live parameters and running statistics on every call: nothing is cached, so in-place edits,
        ``load_state_dict`` and a graph replay always see the current values."""
        w, b = native.bn_fold(weights[-1], biases[-1], norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.eps)
        return [p.detach() for p in weights[:-1]] + [w], [p.detach() if p is not None else None for p in biases[:-1]] + [b]

    def forward_segments(self, segments, residual: Tensor | None = None, rows: int | None = None) -> Tensor:
        """Run the MLP on the virtual concat of ``segments`` = [(table, int32 index | None)]
        (device tensors), optionally adding ``residual``: concat, gathers, Linear chain,
        LayerNorm and residual are one kernel launch.  With ``norm_type='BatchNorm1d'``: in training mode the Linear chain is
        that launch and the batch statistics, the normalisation (+ residual) and their backward run on the K14 kernels; in eval
        mode without a wanted gradient the normalisation is folded into the last Linear and everything is the one launch again."""
        weights, biases, ln = self._kernel_params()
        require_gpu_param(weights[0], "MLP")
        if self.activation_name not in native.ACTIVATIONS:
            raise NotImplementedError(f"activation nn.{self.activation_name} has no HIP kernel "
                                      f"(available: {sorted(native.ACTIVATIONS)})")
        if self.norm_type == "BatchNorm1d":
            return self._forward_batchnorm(weights, biases, self.model[-1], segments, residual, rows)
        return Fn.fused_mlp(segments, weights, biases, ln=ln,
                            activation=self.activation_name, act_param=self._act_param(), residual=residual, rows=rows)

    def _forward_batchnorm(self, weights, biases, norm, segments, residual, rows):
        t0, i0 = segments[0]
        n_rows = int(rows) if rows is not None else int(i0.numel() if i0 is not None else t0.size(0))
        wants_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                                  or any(t.requires_grad for t, _ in segments)
                                                  or (residual is not None and residual.requires_grad))
        kw = dict(activation=self.activation_name, act_param=self._act_param(), rows=rows)
        if n_rows > 0 and self._batchnorm_in_library(norm):
            if norm.training:
                if n_rows == 1:  # torch.nn.functional.batch_norm's check, before any launch
                    raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                                     f"{torch.Size([1, norm.num_features])}")
                z = Fn.fused_mlp(segments, weights, biases, ln=None, residual=None, **kw)
                y = Fn.batch_norm_rows(z, norm.weight, norm.bias, residual, norm.running_mean, norm.running_var, norm.momentum,
                                       norm.eps, True, inplace=True)  # z is this call's own table
                norm.num_batches_tracked.add_(1)  # a device op: no host value enters a captured step
                return y
            if not wants_grad:
                return Fn.fused_mlp(segments, *self._folded_batchnorm(weights, biases, norm), ln=None, residual=residual, **kw)
        # every other case (eval mode with a wanted gradient, no rows, a non-default BatchNorm1d): the PyTorch-ROCm module
        y = Fn.fused_mlp(segments, weights, biases, ln=None, residual=None, **kw)
        y = norm(y)
        if residual is not None:
            y = y + residual
        return y

    def forward_edge_features(self, pos: Tensor, src: Tensor, dst: Tensor) -> Tensor | None:
        """This MLP on the edge features of models/GNN.py:299-302 WITHOUT storing them (K6 as the launch's prologue); None
        when that form is not available (training, a BatchNorm the fold does not serve, a shape / batch size no kernel serves
        this way)."""
        if self.activation_name != "ReLU":
            return None
        if torch.is_grad_enabled() and (pos.requires_grad or any(p.requires_grad for p in self.parameters())):
            return None  # the backward needs the feature rows (dW_0)
        weights, biases, ln = self._kernel_params()
        if self.norm_type == "BatchNorm1d":  # eval mode: folded into the last Linear; training mode needs the batch statistics
            norm = self.model[-1]
            if norm.training or not self._batchnorm_in_library(norm) or not weights[0].is_cuda:
                return None
            weights, biases = self._folded_batchnorm(weights, biases, norm)
        return native.mlp_forward_edge_features(pos, src, dst, weights, biases, ln=ln)

    def forward(self, x: Tensor):
        """models/MLP.py:45-47: flatten to (rows, -1), cast to float32, run the Sequential."""
        dev = require_gpu_param(self.model[0].weight, "MLP")
        src_device = x.device
        x = x.view(x.size(0), -1).to(device=dev, dtype=torch.float32)
        y = self.forward_segments([(x, None)])
        return y if src_device == dev else y.to(src_device)
