"""Inputs, the float64 definition and the bars of the flat Adam update (csrc/optimizer.hip: ``gnc_adam_step_f32`` and the
double-precision entry ``native.adam_step`` calls; tests/test_gpu_adam.py on the GPU, tests/test_adam_host.py on the host).

Definition.  ``adam64``: one step of torch.optim.Adam (amsgrad off, maximize off) in float64, as in the header comment of
optimizer.hip.  The GPU test compares ONE step at a time, from the kernel's own fp32 (p, m, v) and counter, so a bar is one
step's rounding and not the drift of a run.

Bars.  ``adam_fp32`` repeats ``adam_one``'s documented operation order in NumPy fp32 (a fused multiply-add as one rounding of
the float64 result; the two tick scalars and the weights 1 - beta rounded once from Python doubles).  Per element,
|kernel - adam64| must stay within BAR_FACTOR x the larger of |adam_fp32 - adam64| at that element and one fp32 ulp of the
reference value.  The emulation's error is the reference's, not the kernel's.  Measured on the CPU over SIZES (and
256 * 8 * 1024 + 1027) x STEPS steps (``python -m tests.adam_cases``), the largest emulation error of an element as a fraction
of the largest magnitude among its result and operands (p; m, g, wd p; v, g^2, (wd p)^2 - a fraction of the result alone says
nothing where g ~ -wd p or m' ~ 0 cancel):
  wd 0     betas (0.9, 0.999)   p 5.2e-7   m 5.9e-8   v 1.3e-7        betas (0.5, 0.9)   p 5.3e-7   m 5.9e-8   v 1.3e-7
  wd 0.01  betas (0.9, 0.999)   p 7.8e-6   m 6.3e-8   v 1.3e-7        betas (0.5, 0.9)   p 7.8e-6   m 1.4e-7   v 1.3e-7
m and v are one or two roundings.  p is an element with |p| < 1e-3 moved by an update of 1e-3 that carries the four roundings
of sqrt, /, + and /; with weight decay, g + wd p cancels to the size of eps in a few of the 2 M elements and m / (sqrt(v) + eps)
magnifies the rounding of that sum.  (With ``1.f - beta`` formed in fp32, as the kernel did before these tests, v's increment
was 1.3e-5 off at beta2 = 0.999 and p 1.4e-5.)"""
from __future__ import annotations

import math

import numpy as np

SIZES = (1, 3, 4, 5, 1023, 1024, 1027, 4099)  # and num_cu * 8 * 1024 + 1027 on the GPU: the grid-stride loop's second pass + tail
HYPER = tuple((wd, betas) for wd in (0.0, 0.01) for betas in ((0.9, 0.999), (0.5, 0.9)))
LR, EPS = 1e-3, 1e-8
STEPS = 6
BAR_FACTOR = 4.0
G_MIN, G_MAX = 1e-15, 1e15  # g * g neither overflows nor goes subnormal in fp32: float64 and fp32 agree on the semantics
TICK_STEPS = (1, 2, 1000, 10 ** 6, 2 ** 31 + 5)
f32 = np.float32


def hyper_id(h) -> str:
    return f"wd{h[0]}-b{h[1][0]}-{h[1][1]}"


def params(n: int, seed: int = 0) -> np.ndarray:
    """p ~ N(0, 1), float32 [n]."""
    return np.random.default_rng(1000 + seed).standard_normal(n).astype(f32)


def gradient(n: int, step: int, seed: int = 0) -> np.ndarray:
    """The gradient of step ``step`` (0-based): N(0, 1) * 10^(step % 5 - 3), |g| kept within [G_MIN, G_MAX], and every 7th
    element (index % 7 == 0, the same elements on every step) exactly 0."""
    g = np.random.default_rng(7919 * (step + 1) + seed).standard_normal(n) * 10.0 ** (step % 5 - 3)
    g = np.copysign(np.clip(np.abs(g), G_MIN, G_MAX), g).astype(f32)
    g[::7] = 0.0
    return g


def adam64(p, g, m, v, t, lr, b1, b2, eps, wd):
    """(p', m', v') of step number ``t`` (1-based) in float64."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    den = np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps
    return p - (lr / (1.0 - b1 ** t)) * (m / den), m, v


def tick_scalars(t, lr, b1, b2):
    """(step_size, bias_correction2_sqrt) of step ``t`` as float32, from Python doubles."""
    return f32(lr / (1.0 - b1 ** t)), f32(math.sqrt(1.0 - b2 ** t))


def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def adam_fp32(p, g, m, v, t, lr, b1, b2, eps, wd):
    """(p', m', v') by ``adam_one``'s operation order in fp32: every line one rounding."""
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    step_size, bc2_sqrt = tick_scalars(t, lr, b1, b2)
    omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)  # the double difference rounded once, as ATen rounds the scalar Python hands it
    b2, eps, wd = f32(b2), f32(eps), f32(wd)
    if wd != 0:
        g = _fma(wd, p, g)
    m = _fma(omb1, g - m, m)
    v = _fma(omb2 * g, g, v * b2)
    den = np.sqrt(v) / bc2_sqrt + eps
    return _fma(-step_size, m / den, p), m, v


def ulp(x):
    """One fp32 ulp at the magnitude of ``x`` (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(f32)).astype(np.float64)


def bars(p, g, m, v, t, lr, b1, b2, eps, wd):
    """(reference (p', m', v') in float64, their per-element bars, the emulation's errors) for one step from fp32 (p, g, m, v)."""
    ref = adam64(p, g, m, v, t, lr, b1, b2, eps, wd)
    emu = adam_fp32(p, g, m, v, t, lr, b1, b2, eps, wd)
    err = tuple(np.abs(e.astype(np.float64) - r) for e, r in zip(emu, ref))
    return ref, tuple(BAR_FACTOR * np.maximum(e, ulp(r)) for e, r in zip(err, ref)), err


def run_fp32(n: int, hyper, steps: int = STEPS, seed: int = 0):
    """The emulation stepped ``steps`` times from (params, 0, 0): yields (t, inputs of the step, outputs of the step)."""
    wd, (b1, b2) = hyper
    p, m, v = params(n, seed), np.zeros(n, f32), np.zeros(n, f32)
    for s in range(steps):
        g = gradient(n, s, seed)
        out = adam_fp32(p, g, m, v, s + 1, LR, b1, b2, EPS, wd)
        yield s + 1, (p, g, m, v), out
        p, m, v = out


def operand_fractions(p, g, m, v, ref, err, wd):
    """max over the elements of err / (largest magnitude among the result and its operands), for p, m and v."""
    dp = wd * np.asarray(p, dtype=np.float64)
    out = []
    for k, operands in enumerate(((p,), (m, g, dp), (v, np.asarray(g, dtype=np.float64) ** 2, dp * dp))):
        scale = np.maximum.reduce([np.abs(ref[k])] + [np.abs(np.asarray(o, dtype=np.float64)) for o in operands])
        out.append(float((err[k] / np.maximum(scale, 1e-300)).max()))
    return out


if __name__ == "__main__":
    for betas in ((0.9, 0.999), (0.5, 0.9)):
        worst = [0.0] * 3
        for h in (h for h in HYPER if h[1] == betas):
            for n in SIZES + (256 * 8 * 1024 + 1027,):
                for t, (p, g, m, v), _ in run_fp32(n, h):
                    ref, _, err = bars(p, g, m, v, t, LR, *betas, EPS, h[0])
                    worst = [max(a, b) for a, b in zip(worst, operand_fractions(p, g, m, v, ref, err, h[0]))]
        print(betas, "  ".join(f"{name} {w:.1e}" for name, w in zip("pmv", worst)))
