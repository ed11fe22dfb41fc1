"""Shared cases and float64 formulas of the image-MLP tests (K16, the tensor loader, the captured tensor step).

Everything here is written out from the definitions - ``y = x W^T + b``, the activation, LayerNorm over the last dimension, the
chain rule - in float64 on the host; ``test_image_mlp_host.py`` checks it against ``torch.nn`` modules in float64, the GPU tests
check the kernels against it.

Cases are ``(rows, K, H, hidden_layers)`` of ``MLP(K, 2, hidden_dim=H, hidden_layers=hidden_layers)``: K = 1083 = 3 * 19^2 is a row
pitch that is not a multiple of 4 floats; the row counts are 1 row, a short 16-row tile, exact tiles, a tile plus one row and three
tiles with a ragged last one; K = 49152 is the default image, where the split of K runs at its full depth.

Inputs are ``u8 / 255`` values.  Every case records a model seed and an input seed under which ALL hidden pre-activations of the
float64 model stay at least ``RELU_MARGIN`` away from zero, so that no fp32 rounding can flip a ReLU against the reference and no
row of any case needs to be excused; ``test_image_mlp_host.py`` asserts the margin.  The same seeds keep the LayerNorm over the TWO
logits well conditioned: its ``rstd = 1 / sqrt(var + eps)`` multiplies whatever error the logits carry, and two logits that nearly
tie give rstd in the hundreds (model seed 2 of the default-image case: 290, where the row-tiled kernels and K16, each within 2e-7 of
the float64 logits, end 1.4e-5 apart behind the norm).  Two fp32 paths that are each ~1e-7 from the exact logits differ by ~2e-7;
``LN_GAIN_MAX = 25`` keeps that below half of the 1e-5 forward bound.  The seeds were found by ``find_seeds()``
(``python tests/image_mlp_cases.py``): model seeds 0, 1, 2, ... with the input seed fixed at 77, first hit recorded.
"""
from __future__ import annotations

import math

import torch

RELU_MARGIN = 1e-5
LN_GAIN_MAX = 25.0
INPUT_SEED = 77

# (rows, K, H, hidden_layers) -> model seed (see find_seeds)
SHAPES = [(1, 1083, 128, 2), (5, 1083, 40, 2), (8, 1200, 128, 2), (16, 1200, 64, 5), (17, 3072, 128, 2), (33, 3072, 256, 2),
          (64, 3072, 128, 2), (8, 49152, 128, 2), (8, 49152, 128, 5)]
MODEL_SEEDS = {}  # filled below


def case_id(case) -> str:
    return "r{}_k{}_h{}_l{}".format(*case)


def reference_mlp(case, activation: str = "ReLU", norm_type: str | None = "LayerNorm", seed: int | None = None):
    """``MLP(K, 2, H, hidden_layers)`` of this package built on the host under the case's model seed: the reference's module order
    and initialisation (the draws depend on neither the activation nor the norm).  Parameters stay where the class puts them."""
    from graphnet_classifier_amd.MLP import MLP
    rows, K, H, layers = case
    torch.manual_seed(MODEL_SEEDS[case] if seed is None else seed)
    return MLP(K, 2, hidden_dim=H, hidden_layers=layers, activation=activation, norm_type=norm_type)


def params64(model):
    """(weights, biases, gamma | None, beta | None, eps) of an MLP as float64 host tensors."""
    lin = [m for m in model.model if isinstance(m, torch.nn.Linear)]
    norm = model.model[-1] if isinstance(model.model[-1], torch.nn.LayerNorm) else None
    w = [m.weight.detach().double().cpu() for m in lin]
    b = [m.bias.detach().double().cpu() for m in lin]
    if norm is None:
        return w, b, None, None, 0.0
    return w, b, norm.weight.detach().double().cpu(), norm.bias.detach().double().cpu(), float(norm.eps)


def inputs(case, seed: int = INPUT_SEED) -> torch.Tensor:
    """float32 [rows, K] of u8 / 255 values (exactly what ToTensor produces)."""
    rows, K = case[0], case[1]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (rows, K), generator=g, dtype=torch.uint8).float().div(255)


def cotangent(case, width: int = 2, seed: int = 5) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed + case[0])
    return torch.randn(case[0], width, generator=g, dtype=torch.float32)


# ---------------------------------------------------------------- the formulas (float64)
def act(z: torch.Tensor, name: str) -> torch.Tensor:
    if name == "ReLU":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if name == "Identity":
        return z
    if name == "GELU":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    raise KeyError(name)


def act_grad(z: torch.Tensor, name: str) -> torch.Tensor:
    if name == "ReLU":
        return (z > 0).to(z.dtype)
    if name == "Identity":
        return torch.ones_like(z)
    if name == "GELU":
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    raise KeyError(name)


def forward64(x, w, b, gamma, beta, eps, activation: str = "ReLU"):
    """(out, pre-activations z_0 .. z_{L-1}, normalised rows y_hat | None, rstd | None) of the MLP in float64."""
    h, zs = x.double(), []
    for k in range(len(w)):
        z = h @ w[k].t() + b[k]
        zs.append(z)
        h = act(z, activation) if k + 1 < len(w) else z
    if gamma is None:
        return h, zs, None, None
    mean = h.mean(dim=1, keepdim=True)
    var = ((h - mean) ** 2).mean(dim=1, keepdim=True)  # biased, as nn.LayerNorm
    rstd = 1.0 / torch.sqrt(var + eps)
    yhat = (h - mean) * rstd
    return yhat * gamma + beta, zs, yhat, rstd


def backward64(x, w, b, gamma, beta, eps, grad_out, activation: str = "ReLU"):
    """Analytic gradients of ``sum(out * grad_out)``: {"w": [dW_k], "b": [db_k], "gamma", "beta"} in float64."""
    out, zs, yhat, rstd = forward64(x, w, b, gamma, beta, eps, activation)
    g = grad_out.double()
    grads = {"w": [None] * len(w), "b": [None] * len(w), "gamma": None, "beta": None}
    if gamma is not None:
        grads["gamma"] = (g * yhat).sum(dim=0)
        grads["beta"] = g.sum(dim=0)
        gg = g * gamma
        dz = rstd * (gg - gg.mean(dim=1, keepdim=True) - yhat * (gg * yhat).mean(dim=1, keepdim=True))
    else:
        dz = g
    for k in range(len(w) - 1, -1, -1):
        a_in = x.double() if k == 0 else act(zs[k - 1], activation)
        grads["w"][k] = dz.t() @ a_in
        grads["b"][k] = dz.sum(dim=0)
        if k > 0:
            dz = (dz @ w[k]) * act_grad(zs[k - 1], activation)
    return grads


def min_hidden_margin(x, w, b) -> float:
    """Smallest |pre-activation| over every hidden layer of the float64 ReLU model."""
    _, zs, _, _ = forward64(x, w, b, None, None, 0.0, "ReLU")
    return min(float(z.abs().min()) for z in zs[:-1])


def max_layer_norm_gain(x, w, b, eps: float = 1e-5) -> float:
    """Largest rstd of the LayerNorm over the logits of the float64 ReLU model: the factor by which the norm multiplies an error of
    the logits."""
    _, _, _, rstd = forward64(x, w, b, torch.ones(w[-1].size(0), dtype=torch.float64), torch.zeros(w[-1].size(0), dtype=torch.float64), eps)
    return float(rstd.max())


def to_tensor64(u8_hwc: torch.Tensor) -> torch.Tensor:
    """ToTensor from its definition: out[c, y, x] = u8[y, x, c] / 255 (float64; the float32 rounding of it is what the kernel and
    torchvision store: 255 and every uint8 are exact in float32 and IEEE division is correctly rounded)."""
    return u8_hwc.double().permute(2, 0, 1) / 255.0


def find_seeds(limit: int = 400):
    """The first model seed per shape under which the float64 hidden pre-activations keep RELU_MARGIN and the LayerNorm over the
    logits stays below LN_GAIN_MAX (input seed INPUT_SEED)."""
    found = {}
    for case in SHAPES:
        x = inputs(case)
        for seed in range(limit):
            w, b, *_ = params64(reference_mlp(case, seed=seed))
            if min_hidden_margin(x, w, b) >= RELU_MARGIN and max_layer_norm_gain(x, w, b) <= LN_GAIN_MAX:
                found[case] = seed
                break
        else:
            raise RuntimeError(f"no seed below {limit} for {case}")
    return found


MODEL_SEEDS.update({
    (1, 1083, 128, 2): 2, (5, 1083, 40, 2): 1, (8, 1200, 128, 2): 0, (16, 1200, 64, 5): 0, (17, 3072, 128, 2): 9,
    (33, 3072, 256, 2): 0, (64, 3072, 128, 2): 9, (8, 49152, 128, 2): 3, (8, 49152, 128, 5): 4,
})
CASES = list(SHAPES)

if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for c, s in find_seeds().items():
        print(f"    {c}: {s},")
