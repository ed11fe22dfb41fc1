"""Inputs, float64 definitions and bars of the controlled optimizer step (csrc/optimizer_ctl.hip, DESIGN K22; the GPU tests are
tests/test_gpu_optimizer_controls.py, the host side tests/test_optimizer_controls_host.py).  Parameters and gradients are the
recipe of tests/adam_cases.py.

Definitions, all float64.  ``lr_at``: linear warm-up, then constant / cosine / step.  ``clip_coef64``: ``clip_grad_norm_``'s
``min(1, max_norm / (norm + 1e-6))`` over the whole gradient.  ``adamw64``: ``p *= 1 - lr * wd``, then Adam without L2
(torch.optim.AdamW).  ``sgd64``: ``g += wd p; buf = mu buf + g; d = g + mu buf | buf; p -= lr d`` (torch.optim.SGD, dampening 0; a
zero ``buf`` gives torch's first-step ``buf = g``).  ``step64`` applies ``g <- clip_coef * g`` and then the rule.  The GPU test
compares ONE step at a time from the kernel's own fp32 state, so a bar is one step's rounding and not the drift of a run.

Bars.  ``step_fp32`` repeats the operation order documented in optimizer_ctl.hip in NumPy fp32: the tick's scalars (lr, step
size, decay, clip coefficient) rounded once from float64, ``g = fl(coef * g)``, then one rounding per line of the rule.  Per
element, |kernel - float64| must stay within BAR_FACTOR x the larger of |emulation - float64| at that element and one fp32 ulp of
the reference value - the project's bar, BAR_FACTOR of adam_cases.  Measured on the CPU over SIZES x STEPS steps x wd in
(0, 0.01) x the three clip settings (``python -m tests.optimizer_control_cases``), the largest emulation error of an element as a
fraction of the largest magnitude among its result and operands:
  adam            p 2.8e-07   m 5.8e-08   v 1.3e-07
  adamw           p 2.8e-07   m 5.8e-08   v 1.2e-07
  sgd             p 7.1e-08
  sgd_momentum    p 9.1e-08   buf 1.5e-07
  sgd_nesterov    p 6.8e-08   buf 1.5e-07
Each is a handful of fp32 roundings (6e-8 apiece); adam_cases' rare cancellation of g + wd p to the size of eps does not occur in
sizes this small.  The host test holds the emulation to 1e-6 for p and 3e-7 for the state tensors."""
from __future__ import annotations

import math

import numpy as np

from tests import adam_cases as A

f32 = np.float32
SIZES = (5, 1027, 4099)  # n < one float4 + tail; four blocks + tail; and (GPU only) the element grid's second pass
STEPS = A.STEPS
LR, EPS, BETAS = A.LR, A.EPS, (0.9, 0.999)
WDS = (0.0, 0.01)
RULES = {  # name: (rule of native.opt_ctl, momentum, nesterov)
    "adam": ("adam", 0.0, False), "adamw": ("adamw", 0.0, False), "sgd": ("sgd", 0.0, False),
    "sgd_momentum": ("sgd", 0.9, False), "sgd_nesterov": ("sgd", 0.9, True),
}
# the gradients of the recipe have norms from 1e-3 * sqrt(n) to 10 * sqrt(n): 1e-3 bites on every step of every n >= 1023, 1e9 on none
CLIPS = {"noclip": None, "bites": 1e-3, "loose": 1e9}
SCHEDULE = dict(kind="cosine", warmup_steps=2, total_steps=5, min_lr=1e-5)  # 6 steps: warm-up, decay, the end value and its hold
TICK_STEPS = (1, 10, 11, 50, 55, 10 ** 6)  # t in {1, warmup, warmup + 1, total, total + 5, 10^6} of TICK_SCHEDULES
TICK_SCHEDULES = (dict(kind="cosine", warmup_steps=10, total_steps=50, min_lr=1e-6),
                  dict(kind="step", warmup_steps=10, total_steps=50, gamma=0.5, every=7),
                  dict(kind="constant", warmup_steps=10, total_steps=50))


def lr_at(t, lr, kind="constant", warmup_steps=0, total_steps=0, min_lr=0.0, gamma=0.1, every=1):
    """Learning rate of optimizer step ``t`` (1-based)."""
    if t <= warmup_steps:
        return lr * (float(t) / float(warmup_steps))  # exactly lr at t == warmup_steps
    if kind == "cosine":
        if t >= total_steps:
            return min_lr
        return min_lr + 0.5 * (lr - min_lr) * (1.0 + math.cos(math.pi * (float(t - warmup_steps) / float(total_steps - warmup_steps))))
    if kind == "step":
        return lr * gamma ** float((t - warmup_steps) // every)
    assert kind == "constant", kind
    return lr


def norm64(g) -> float:
    g = np.asarray(g, dtype=np.float64)
    return math.sqrt(float(np.sum(g * g)))  # pairwise in float64: 1e-15 of itself, nine digits below an fp32 ulp


def clip_coef64(g, max_norm) -> float:
    return 1.0 if max_norm is None else min(1.0, max_norm / (norm64(g) + 1e-6))


def adamw64(p, g, m, v, t, lr, b1, b2, eps, wd):
    """(p', m', v') of step ``t`` of torch.optim.AdamW in float64."""
    p = np.asarray(p, dtype=np.float64) * (1.0 - lr * wd)
    return A.adam64(p, g, m, v, t, lr, b1, b2, eps, 0.0)


def sgd64(p, g, buf, lr, mu, wd, nesterov):
    """(p', buf') of torch.optim.SGD in float64; ``buf`` is None without momentum."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    g = g + wd * p
    d = g
    if mu != 0:
        buf = np.asarray(buf, dtype=np.float64) * mu + g
        d = g + mu * buf if nesterov else buf
    return p - lr * d, buf


def tick64(rule, t, lr_t, wd, coef, b1=BETAS[0], b2=BETAS[1]):
    """The tick's scalars in float64: (step_size, bc2_sqrt, decay, clip_coef, lr)."""
    if rule == "sgd":
        return lr_t, 1.0, 1.0, coef, lr_t
    return lr_t / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), (1.0 - lr_t * wd) if rule == "adamw" else 1.0, coef, lr_t


def step64(name, state, g, t, lr_t, wd, max_norm):
    """One controlled step in float64 from ``state`` = (p, m, v) or (p, buf) or (p,): the new state, same layout."""
    rule, mu, nesterov = RULES[name]
    g = clip_coef64(g, max_norm) * np.asarray(g, dtype=np.float64)
    if rule == "adam":
        return A.adam64(*state[:1], g, *state[1:], t, lr_t, *BETAS, EPS, wd)
    if rule == "adamw":
        return adamw64(*state[:1], g, *state[1:], t, lr_t, *BETAS, EPS, wd)
    p, buf = sgd64(state[0], g, state[1] if mu else None, lr_t, mu, wd, nesterov)
    return (p, buf) if mu else (p,)


def step_fp32(name, state, g, t, lr_t, wd, max_norm):
    """The same step by the kernel's documented operation order in fp32: every line one rounding."""
    rule, mu, nesterov = RULES[name]
    state = tuple(np.asarray(a, dtype=f32) for a in state)
    g = f32(clip_coef64(g, max_norm)) * np.asarray(g, dtype=f32)
    if rule == "adam":
        return A.adam_fp32(state[0], g, state[1], state[2], t, lr_t, *BETAS, EPS, wd)
    if rule == "adamw":
        return A.adam_fp32(state[0] * f32(1.0 - lr_t * wd), g, state[1], state[2], t, lr_t, *BETAS, EPS, 0.0)
    p = state[0]
    if wd != 0:
        g = A._fma(f32(wd), p, g)
    d = g
    out = ()
    if mu != 0:
        buf = state[1] * f32(mu) + g  # two roundings: mul_, add_
        d = A._fma(f32(mu), buf, g) if nesterov else buf
        out = (buf,)
    return (A._fma(-f32(lr_t), d, p),) + out


def bars(name, state, g, t, lr_t, wd, max_norm):
    """(float64 reference state, per-element bars, the emulation's errors) for one step from the fp32 ``state``."""
    ref = step64(name, state, g, t, lr_t, wd, max_norm)
    emu = step_fp32(name, state, g, t, lr_t, wd, max_norm)
    err = tuple(np.abs(e.astype(np.float64) - r) for e, r in zip(emu, ref))
    return ref, tuple(A.BAR_FACTOR * np.maximum(e, A.ulp(r)) for e, r in zip(err, ref)), err


def initial_state(name, n, seed=0):
    rule, mu, _ = RULES[name]
    zeros = 2 if rule != "sgd" else (1 if mu else 0)
    return (A.params(n, seed),) + tuple(np.zeros(n, f32) for _ in range(zeros))


def run_fp32(name, n, wd, max_norm, steps=STEPS, schedule=SCHEDULE):
    """The emulation stepped from (params, zero state): yields (t, lr(t), gradient, state before, state after)."""
    state = initial_state(name, n)
    for s in range(steps):
        g, lr_t = A.gradient(n, s), lr_at(s + 1, LR, **schedule)
        out = step_fp32(name, state, g, s + 1, lr_t, wd, max_norm)
        yield s + 1, lr_t, g, state, out
        state = out


def operand_fractions(name, state, g, ref, err, wd, max_norm):
    """max over the elements of err / (largest magnitude among the result and its operands), for every state tensor."""
    g = clip_coef64(g, max_norm) * np.asarray(g, dtype=np.float64)
    dp = wd * np.asarray(state[0], dtype=np.float64)
    if RULES[name][0] == "sgd":
        operands = ((state[0],), (state[-1], g, dp))
    else:
        operands = ((state[0],), (state[1], g, dp), (state[2], g * g, dp * dp))
    out = []
    for k in range(len(state)):
        scale = np.maximum.reduce([np.abs(ref[k])] + [np.abs(np.asarray(o, dtype=np.float64)) for o in operands[k]])
        out.append(float((err[k] / np.maximum(scale, 1e-300)).max()))
    return out


def worst_fractions(name, sizes=SIZES):
    worst = [0.0] * len(initial_state(name, 1))
    for wd in WDS:
        for max_norm in CLIPS.values():
            for n in sizes:
                for t, lr_t, g, state, _ in run_fp32(name, n, wd, max_norm):
                    ref, _, err = bars(name, state, g, t, lr_t, wd, max_norm)
                    worst = [max(a, b) for a, b in zip(worst, operand_fractions(name, state, g, ref, err, wd, max_norm))]
    return worst


if __name__ == "__main__":
    for rule_name in RULES:
        labels = ("p", "m", "v") if RULES[rule_name][0] != "sgd" else ("p", "buf")
        print(f"{rule_name:15s}", "   ".join(f"{label} {w:.1e}" for label, w in zip(labels, worst_fractions(rule_name))))
