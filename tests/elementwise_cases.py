"""Inputs, float64 definitions and bars of the row-wise kernels of csrc/elementwise.hip (tests/test_gpu_elementwise.py on the
GPU; tests/test_mlp_family_cases_host.py checks on the host that the same fp32 formulas meet the bars).

Activations and derivatives.  One input table: a linear grid on [-30, 30], +-logspace(1e-8, 1e-1) (where ``expf(x) - 1`` and
its kin lose their digits), +-0, +-88 and +-100 (``expf(-x)`` overflows).  Its length is a multiple of every tested width.
  ABS_BAR  |err| <= 4e-7 * max(1, |x|) everywhere
  REL_BAR  |err| <= 1e-6 * |ref| for |x| <= 1e-2 where ref != 0
The fp32 formulas of the kernels, evaluated on the CPU, give at most 1.2e-7 and 2.2e-7 of these; the margin of about 4 x is for
the device's tanhf, erff and expf."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import mlp_family_cases as M

ACTS = tuple(M.ACT_PARAM.items())  # (name, parameter): Tanh, Sigmoid, SiLU, GELU, LeakyReLU 0.01, ELU 1.0
WIDTHS = (1, 3, 64, 100, 256)
TABLE_LEN = 19200  # lcm(3, 64, 100, 256)
ABS_BAR = 4e-7
REL_BAR = 1e-6
REL_RANGE = 1e-2
GRAD_SCALES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)  # powers of two: da * act'(z) rounds exactly as act'(z) does


@functools.lru_cache(maxsize=None)
def table() -> torch.Tensor:
    """The float32 input table, [TABLE_LEN]; the special values are spread over it, not bunched at one end."""
    small = np.logspace(-8, -1, 297)
    special = np.array([0.0, -0.0, 88.0, -88.0, 100.0, -100.0])
    grid = np.linspace(-30.0, 30.0, TABLE_LEN - 2 * small.size - special.size)
    x = np.concatenate([grid, small, -small, special]).astype(np.float32)
    assert x.size == TABLE_LEN
    return torch.from_numpy(np.random.default_rng(7).permutation(x))


def grad_table(n: int) -> torch.Tensor:
    """Incoming gradients for ``n`` elements: signs and scales vary, so a gradient read from the wrong place shows."""
    return torch.tensor(GRAD_SCALES, dtype=torch.float32)[torch.from_numpy(np.random.default_rng(11).integers(0, 6, n))]


def reference(x: torch.Tensor, name: str, param: float):
    """(act(x), act'(x)) in float64: the torch.nn.functional definition and its autograd."""
    z = x.double().clone().requires_grad_(True)
    a = M.activate(z, name, param)
    a.sum().backward()
    return a.detach(), z.grad


def fp32_formulas(x: torch.Tensor, name: str, p: float):
    """(act(x), act'(x)) by the kernels' own formulas (act_fwd / act_grad of csrc/elementwise.hip) in fp32 on the CPU."""
    x = x.float()
    one = torch.ones_like(x)
    s = 1.0 / (1.0 + torch.exp(-x))
    if name == "Tanh":
        t = torch.tanh(x)
        return t, 1.0 - t * t
    if name == "Sigmoid":
        return s, s * (1.0 - s)
    if name == "SiLU":
        return x / (1.0 + torch.exp(-x)), s * (1.0 + x * (1.0 - s))
    if name == "GELU":
        cdf = 0.5 * (1.0 + torch.erf(x * np.float32(0.70710678118654752440)))
        pdf = np.float32(0.39894228040143267794) * torch.exp(-0.5 * x * x)
        return 0.5 * x * (1.0 + torch.erf(x * np.float32(0.70710678118654752440))), cdf + x * pdf
    if name == "LeakyReLU":
        return torch.where(x < 0, x * np.float32(p), x), torch.where(x > 0, one, one * np.float32(p))
    if name == "ELU":
        return torch.where(x > 0, x, np.float32(p) * torch.expm1(x)), torch.where(x > 0, one, np.float32(p) * torch.exp(x))
    raise KeyError(name)


def errors(got: torch.Tensor, ref: torch.Tensor, x: torch.Tensor, scale: torch.Tensor | None = None) -> dict:
    """Both figures of a result against its float64 reference, each as a fraction of its bar's unit (``abs``: of max(1, |x|);
    ``rel``: of |ref| on |x| <= REL_RANGE where ref != 0), and whether every value is finite.  ``scale``: the |gradient| that
    multiplied result and reference exactly."""
    got, ref, x = got.double().flatten(), ref.double().flatten(), x.double().flatten()
    err = (got - ref).abs()
    if scale is not None:
        err, ref = err / scale.double().flatten().abs(), ref / scale.double().flatten().abs()
    near = (x.abs() <= REL_RANGE) & (ref != 0)
    return {"abs": float((err / x.abs().clamp_min(1.0)).max()),
            "rel": float((err[near] / ref[near].abs()).max()) if bool(near.any()) else 0.0,
            "finite": bool(torch.isfinite(got).all())}


# ------------------------------------------------------------------------------------------------ LayerNorm backward
LN_WIDTHS = (1, 3, 32, 64, 65, 100, 128, 200, 256)
LN_HARD_WIDTHS = (3, 65, 100, 256)  # the widths of the ``offset`` and ``constant`` inputs
LN_EPS = M.LN_EPS
# Bars.  ``normal`` inputs: dy under M.DX_BAR (absolute), y_hat under M.TOL * max(1, max|ref|); plain fp32 on the CPU (ln_fp32) is
# 2.0e-6 / 8.3e-7 off float64 there at 16,421 rows.  The other two kinds are beyond absolute bars of that size in fp32 itself,
# whatever the formula (figures: ln_fp32 against float64 at widths 3 / 65 / 100 / 256 and 1, 37 and 16,421 rows; autograd of
# F.layer_norm in fp32 on the CPU gives 1.3e-3 / 2.7e-4 and 3.1e-4):
#   offset    rows around 1e3 carry 6e-5 of rounding in the mean alone: dy 8.05e-4, y_hat 2.81e-4
#   constant  rstd = 1 / sqrt(eps) = 316 and |dy| reaches 2.4e3:        dy 2.74e-4 (y_hat is exactly 0: TOL stays)
# so there the bar is 3 x the fp32-CPU figure, as for M.LN_SUM_BAR_LOOP.
LN_FP32_CPU = {"offset": (8.05e-4, 2.81e-4), "constant": (2.74e-4, None)}


def ln_bars(kind: str, yhat_ref: torch.Tensor) -> tuple:
    """(bar of dy, bar of y_hat) for inputs of ``kind``."""
    dy_fig, yh_fig = LN_FP32_CPU.get(kind, (None, None))
    return (3 * dy_fig if dy_fig else M.DX_BAR, 3 * yh_fig if yh_fig else M.TOL * max(1.0, float(yhat_ref.abs().max())))


def ln_inputs(rows: int, width: int, kind: str = "normal"):
    """(y, gamma, grad_out) float32 on the CPU.  ``normal``: every row has its own mean in [-1, 1] and its own standard
    deviation in [0.5, 2] (set exactly, so that no row of a narrow table is degenerate by chance: rstd stays of order 1 and the
    absolute bars mean something); ``offset``: the same around 1e3 (a mean far larger than the spread); ``constant``: every
    row a constant (variance 0: eps alone decides rstd), the constants small integers, whose sums are exact."""
    rng = np.random.default_rng(1000 * width + rows % 1000 + {"normal": 0, "offset": 1, "constant": 2}[kind])
    y = rng.standard_normal((rows, width))
    if width > 1:
        y = (y - y.mean(axis=1, keepdims=True)) / y.std(axis=1, keepdims=True)
    y = rng.uniform(-1.0, 1.0, (rows, 1)) + rng.uniform(0.5, 2.0, (rows, 1)) * y
    if kind == "offset":
        y = 1e3 + y
    elif kind == "constant":
        y = np.repeat(rng.integers(-4, 5, (rows, 1)).astype(np.float64), width, axis=1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return f32(y), f32(rng.uniform(0.5, 1.5, width)), f32(rng.standard_normal((rows, width)))


def ln_fp32(y, gamma, grad_out):
    """(dy, y_hat) by the two-pass textbook formulas in plain fp32 on the CPU: the yardstick where fp32 arithmetic itself
    cannot meet an absolute bar (a mean of 1e3, rstd = 316 on a constant row)."""
    inv_n = np.float32(1.0 / y.size(1))
    d = y - y.sum(1, keepdim=True) * inv_n
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) * inv_n + np.float32(LN_EPS))
    yhat, gg = d * rstd, grad_out * gamma
    return rstd * (gg - gg.sum(1, keepdim=True) * inv_n - yhat * ((gg * yhat).sum(1, keepdim=True) * inv_n)), yhat


def ln_reference(y, gamma, grad_out, dtype=torch.float64):
    """(dy, y_hat) of out = LayerNorm(y) * gamma + beta: autograd of F.layer_norm in ``dtype``."""
    yy = y.to(dtype).clone().requires_grad_(True)
    w = y.size(1)
    out = torch.nn.functional.layer_norm(yy, (w,), gamma.to(dtype), torch.zeros(w, dtype=dtype), LN_EPS)
    out.backward(grad_out.to(dtype))
    with torch.no_grad():
        yhat = torch.nn.functional.layer_norm(yy, (w,), None, None, LN_EPS)
    return yy.grad, yhat.detach()
