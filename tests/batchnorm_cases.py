"""Float64 formulas, inputs and references of the batch-norm (K14) tests: tests/test_gpu_batchnorm.py on the GPU,
tests/test_batchnorm_host.py on the host, where the formulas themselves are pinned to ``torch.nn.BatchNorm1d`` in float64
and to the golden vectors captured from the reference (tests/golden/g11_batchnorm.npz).  A data set is built once per process
and shared read-only.

Everything here is written out from the definition (models/MLP.py:29-35 appends ``nn.BatchNorm1d(out_dim)``):
training mode normalises with the batch mean and the BIASED batch variance, updates the running statistics with the
UNBIASED one; eval mode normalises with the running statistics."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import graphnet_oracle as O

EPS, MOMENTUM = 1e-5, 0.1
ROWS = (2, 17, 63, 64, 65, 4099)       # + the two row counts taken from gnc_bn_partials on the device
SMALL_EDGE = (4096, 4097)              # the last row count of the one-launch kernels (gnc_bn_small_max_rows) and the first above
WIDTHS = (1, 5, 20, 64, 130, 256)


# ------------------------------------------------------------------------------------------------------------ formulas
def stats(z: torch.Tensor):
    """(mean, biased variance) per column, two passes."""
    mean = z.mean(dim=0)
    return mean, ((z - mean) ** 2).mean(dim=0)


def apply(z, mean, invstd, gamma, beta, residual=None):
    out = (z - mean) * invstd * gamma + beta
    return out if residual is None else out + residual


def forward_train(z, gamma, beta, residual=None, eps=EPS):
    mean, var = stats(z)
    return apply(z, mean, 1.0 / torch.sqrt(var + eps), gamma, beta, residual)


def backward(grad_out, z, gamma, eps=EPS):
    """(dz, dgamma, dbeta, dresidual) of ``forward_train``: closed form, no autograd."""
    rows = z.size(0)
    mean, var = stats(z)
    invstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * invstd
    dbeta = grad_out.sum(dim=0)
    dgamma = (grad_out * xhat).sum(dim=0)
    dz = gamma * invstd * (grad_out - dbeta / rows - xhat * dgamma / rows)
    return dz, dgamma, dbeta, grad_out


def running_update(running_mean, running_var, z, momentum=MOMENTUM):
    rows = z.size(0)
    mean, var = stats(z)
    return ((1 - momentum) * running_mean + momentum * mean,
            (1 - momentum) * running_var + momentum * var * rows / (rows - 1))


def fold(weight, bias, gamma, beta, running_mean, running_var, eps=EPS):
    """(W', b'): Linear(weight, bias) followed by the eval-mode normalisation, as one Linear."""
    s = gamma / torch.sqrt(running_var + eps)
    return s[:, None] * weight, s * bias + beta - running_mean * s


# ------------------------------------------------------------------------------------------------ the reference's modules
def _mlp(sd, prefix, x, training, new_buffers):
    """models/MLP.py:45-47 with a BatchNorm1d (or no norm) at the end, from a state dict; differentiable."""
    idx = sorted({int(k[len(prefix) + 7:].split(".")[0]) for k in sd if k.startswith(prefix + ".model.")})
    lin = [i for i in idx if sd[f"{prefix}.model.{i}.weight"].ndim == 2]
    for n, i in enumerate(lin):
        x = O.linear(x, sd[f"{prefix}.model.{i}.weight"], sd[f"{prefix}.model.{i}.bias"])
        if n + 1 < len(lin):
            x = x.clamp_min(0)
    for i in idx:
        p = f"{prefix}.model.{i}."
        if p + "running_mean" not in sd:
            continue
        gamma, beta, rm, rv = sd[p + "weight"], sd[p + "bias"], sd[p + "running_mean"], sd[p + "running_var"]
        if training:
            with torch.no_grad():
                new_buffers[p + "running_mean"], new_buffers[p + "running_var"] = running_update(rm, rv, x)
                new_buffers[p + "num_batches_tracked"] = sd[p + "num_batches_tracked"] + 1
            x = forward_train(x, gamma, beta)
        else:
            x = apply(x, rm, 1.0 / torch.sqrt(rv + EPS), gamma, beta)
    return x


def graphnet_forward(sd, x, pos, edge_index, training, prefix="graph_net."):
    """GraphNet.forward (models/GNN.py:297-309) of a norm_type='BatchNorm1d' model in the dtype of ``sd``.
    Returns (per-node output, {buffer key: value after the forward}) - the dict is empty in eval mode."""
    dtype = sd[prefix + "node_encoder.model.0.weight"].dtype
    nb = {}
    row, col = edge_index[0], edge_index[1]
    e = _mlp(sd, prefix + "edge_encoder", O.edge_features(pos.to(dtype), edge_index), training, nb)
    h = _mlp(sd, prefix + "node_encoder", x.to(dtype), training, nb)
    for b in range(O.n_blocks_of(sd, prefix)):
        blk = f"{prefix}graph_processor.blocks.{b}"
        e = _mlp(sd, blk + ".edge_model.edge_processor", torch.cat([h[row], h[col], e], -1), training, nb) + e
        agg = torch.zeros(h.size(0), e.size(1), dtype=dtype).index_add(0, col, e)
        h = _mlp(sd, blk + ".node_model.node_processor", torch.cat([h, agg], -1), training, nb) + h
    return _mlp(sd, prefix + "node_decoder", h, training, nb), nb


def combined_train_step(sd32: dict, x, pos, edge_index, label):
    """One training-mode forward + backward of CombinedModel in float64 from a float32 state dict: dict with ``y`` (per-node
    GraphNet output), ``logits``, ``loss``, ``grads`` {parameter key: gradient}, ``buffers`` (after the forward) and, from those
    buffers, ``eval_y`` / ``eval_logits``."""
    sd = O.to_dtype(sd32, torch.float64)
    params = [k for k, v in sd32.items() if v.is_floating_point() and "running_" not in k]
    for k in params:
        sd[k].requires_grad_(True)
    y, buffers = graphnet_forward(sd, x, pos, edge_index, training=True)
    logits = O.classifier_forward(sd, y.flatten())
    loss = torch.nn.functional.cross_entropy(logits[None], label.view(1))
    grads = dict(zip(params, torch.autograd.grad(loss, [sd[k] for k in params])))
    with torch.no_grad():
        sd_after = {**sd, **buffers}
        eval_y, _ = graphnet_forward(sd_after, x, pos, edge_index, training=False)
        eval_logits = O.classifier_forward(sd_after, eval_y.flatten())
    return {"y": y.detach(), "logits": logits.detach(), "loss": loss.detach(), "grads": grads, "buffers": buffers,
            "eval_y": eval_y, "eval_logits": eval_logits}


# ------------------------------------------------------------------------------------------------------------ data sets
@functools.lru_cache(maxsize=None)
def ill_conditioned(rows: int, width: int) -> dict:
    """float32 ``z`` [rows, width] whose column c is, by c % 3: N(0, 1); N(1000, 1); N(1000, 1) with row 0 set to 0 (an outlier
    in the one row a shifted algorithm would take as its shift).  ``mean`` / ``var``: float64 statistics of those float32 values."""
    rng = np.random.default_rng(1000 * width + rows % 997)
    z = rng.standard_normal((rows, width))
    kind = np.arange(width) % 3
    z[:, kind > 0] += 1000.0
    z[0, kind == 2] = 0.0
    z = torch.from_numpy(z.astype(np.float32))
    mean, var = stats(z.double())
    return {"z": z, "mean": mean, "var": var, "colmax": z.abs().amax(dim=0).double()}


@functools.lru_cache(maxsize=None)
def well_conditioned(rows: int, width: int) -> dict:
    """float32 inputs of one forward + backward (column means in [-1, 1], standard deviations in [0.5, 2]) and their float64
    references: ``out`` (with the residual), ``dz`` / ``dgamma`` / ``dbeta``, the running statistics after one update from
    ``running_mean`` / ``running_var``."""
    g = torch.Generator().manual_seed(7919 * width + rows)
    r = lambda *shape: torch.randn(*shape, generator=g)
    u = lambda lo, hi, n: lo + (hi - lo) * torch.rand(n, generator=g)
    z = r(rows, width) * u(0.5, 2.0, width) + u(-1.0, 1.0, width)
    d = {"z": z, "gamma": u(0.5, 1.5, width), "beta": u(-0.5, 0.5, width), "residual": r(rows, width), "grad_out": r(rows, width),
         "running_mean": u(-1.0, 1.0, width), "running_var": u(0.5, 2.0, width)}
    d64 = {k: v.double() for k, v in d.items()}
    d["out"] = forward_train(d64["z"], d64["gamma"], d64["beta"], d64["residual"])
    d["out_plain"] = forward_train(d64["z"], d64["gamma"], d64["beta"])
    d["dz"], d["dgamma"], d["dbeta"], _ = backward(d64["grad_out"], d64["z"], d64["gamma"])
    d["new_running_mean"], d["new_running_var"] = running_update(d64["running_mean"], d64["running_var"], d64["z"])
    return d


def bound(ref: torch.Tensor) -> float:
    """The project's per-tensor bound: absolute, because the bias in front of a BatchNorm has a true gradient of 0."""
    return 2e-5 + 1e-4 * float(ref.abs().max())
