"""Inputs, float64 definitions and bars of the single-graph read-out (csrc/readout.hip: ``gnc_readout_forward_f32`` /
``gnc_readout_backward_f32``; tests/test_gpu_readout.py on the GPU, tests/test_readout_host.py proves definitions and bars on
the host).

Cases.  ``case(F, H1, H2, C, seed)``: w_k ~ N(0, 1) / sqrt(fan_in), b_k ~ 0.1 N(0, 1), y, g ~ N(0, 1), drawn in float64 and
rounded to fp32, so the kernel and the float64 formulas read the same numbers.  SHAPES are the smallest shapes that cross each
loop boundary of the two kernels (256 threads, 64 lanes, 4 waves, the float4 path and its tail, H1 > 256, both maxima).

ReLU kink.  Every case keeps min|z| >= KINK * rms(z) for both pre-activations in float64 (asserted by ``case``; no unit is
masked, a seed that misses is replaced: SEEDS).  Smallest ratio of the nine cases: 3.6e-4 (z2 of 1024x257x1024x63).  The
fp32 forward is 4e-7 of max|z| off at most, so float64 and the kernel agree on every mask and gradients are compared on all
elements.

Bars.  Per case and per output, in max-norm: BAR_FACTOR x the larger of (a) the error of the same formulas evaluated in plain
fp32 on the CPU against float64 and (b) 2^-23 max|ref|.  (a) is the reference's error, not the kernel's; the factor 4 is for
the kernel's other summation order (lane tree, four waves, float4 pairing, ascending in-thread sums of the backward), (b) for
cases where the CPU happens to be exact ((1, 1, 1, 1)).  Measured on the CPU, (a) as a fraction of max|ref| over the nine
cases (``python -m tests.readout_cases`` prints the table):
  logits 2.8e-8 .. 2.8e-7   h1 5.4e-9 .. 4.0e-7   h2 9.5e-9 .. 3.4e-7   dy 1.7e-8 .. 2.9e-7   dW1 1.8e-8 .. 1.6e-7
  db1 2.2e-8 .. 1.6e-7   dW2 1.0e-9 .. 4.5e-7 (2048x1024x96x64)   db2 3.3e-8 .. 1.6e-7   dW3 4.0e-8 .. 3.3e-7   db3 0 (a copy)
so the bars lie between 4.8e-7 (the floor) and 1.8e-6 of max|ref|."""
from __future__ import annotations

import functools

import torch

SHAPES = ((1, 1, 1, 1), (5, 3, 2, 1), (255, 7, 5, 3), (257, 65, 33, 5), (1023, 129, 64, 4), (1028, 128, 32, 2),
          (4096, 128, 32, 2), (2048, 1024, 96, 64), (1024, 257, 1024, 63))
SEEDS = {s: 0 for s in SHAPES}  # seed 0 meets the kink condition at every shape
SEEDS[(1, 1, 1, 1)] = 1  # seed 0 leaves both units off: every gradient would be 0
KINK = 1e-4
BAR_FACTOR = 4.0
ULP = 2.0 ** -23
INPUTS = ("y", "w1", "b1", "w2", "b2", "w3", "b3", "g")
OUTPUTS = ("logits", "h1", "h2")
GRADS = ("dy", "dW1", "db1", "dW2", "db2", "dW3", "db3")
BIAS_SHAPE = (257, 65, 33, 5)  # the shape of the 8 bias combinations, the layouts and the ReLU edges


def case_id(shape) -> str:
    return "x".join(str(v) for v in shape)


def forward64(y, w1, b1, w2, b2, w3, b3):
    """(z1, h1, z2, h2, logits) of logits = fc3(relu(fc2(relu(fc1(y))))) in the dtype of the arguments; a bias may be None."""
    z1 = w1 @ y if b1 is None else w1 @ y + b1
    h1 = torch.where(z1 > 0, z1, torch.zeros_like(z1))
    z2 = w2 @ h1 if b2 is None else w2 @ h1 + b2
    h2 = torch.where(z2 > 0, z2, torch.zeros_like(z2))
    logits = w3 @ h2 if b3 is None else w3 @ h2 + b3
    return z1, h1, z2, h2, logits


def backward64(g, y, w1, w2, w3, h1, h2):
    """(dy, dW1, db1, dW2, db2, dW3, db3) for the cotangent ``g`` of the logits, by formula with the mask ``h > 0``."""
    dz2 = (w3.t() @ g) * (h2 > 0).to(g.dtype)
    dz1 = (w2.t() @ dz2) * (h1 > 0).to(g.dtype)
    return w1.t() @ dz1, torch.outer(dz1, y), dz1, torch.outer(dz2, h1), dz2, torch.outer(g, h2), g.clone()


def kink_ratio(z) -> float:
    """min|z| / rms(z)"""
    return float(z.abs().min() / z.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def case(F: int, H1: int, H2: int, C: int, seed: int) -> dict:
    """fp32-representable float64 tensors y, w1, b1, w2, b2, w3, b3, g (shared: do not write to them)."""
    gen = torch.Generator().manual_seed(seed)
    n = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    c = {"y": n(F), "w1": n(H1, F) / F ** 0.5, "b1": 0.1 * n(H1), "w2": n(H2, H1) / H1 ** 0.5, "b2": 0.1 * n(H2),
         "w3": n(C, H2) / H2 ** 0.5, "b3": 0.1 * n(C), "g": n(C)}
    c = {k: v.float().double() for k, v in c.items()}
    z1, _, z2, _, _ = forward64(*(c[k] for k in INPUTS[:7]))
    assert kink_ratio(z1) >= KINK and kink_ratio(z2) >= KINK, (F, H1, H2, C, seed, kink_ratio(z1), kink_ratio(z2))
    return c


def build(shape) -> dict:
    return case(*shape, SEEDS[tuple(shape)])


def without_biases(c: dict, keep=(False, False, False)) -> dict:
    """``c`` with b_k replaced by None where ``keep[k]`` is false."""
    out = dict(c)
    for name, k in zip(("b1", "b2", "b3"), keep):
        if not k:
            out[name] = None
    return out


def evaluate(c: dict, dtype=torch.float64) -> dict:
    """Every output of forward and backward by the formulas above, computed in ``dtype`` (float64: the reference; float32: the
    plain CPU evaluation whose error sets the bars).  The backward reads the h1, h2 of its own forward, as the kernel does."""
    a = {k: None if v is None else v.to(dtype) for k, v in c.items()}
    z1, h1, z2, h2, logits = forward64(*(a[k] for k in INPUTS[:7]))
    out = {"z1": z1, "z2": z2, "logits": logits, "h1": h1, "h2": h2}
    out.update(zip(GRADS, backward64(a["g"], a["y"], a["w1"], a["w2"], a["w3"], h1, h2)))
    return out


def max_err(got, ref) -> float:
    return float((got.double() - ref.double()).abs().max())


def reference(c: dict) -> dict:
    """{"ref": float64 outputs, "fp32": fp32-CPU outputs, "err": their max-norm distance, "bar": per output} of case ``c``."""
    ref, f32 = evaluate(c, torch.float64), evaluate(c, torch.float32)
    err = {k: max_err(f32[k], ref[k]) for k in OUTPUTS + GRADS}
    bar = {k: BAR_FACTOR * max(err[k], ULP * float(ref[k].abs().max())) for k in OUTPUTS + GRADS}
    return {"ref": ref, "fp32": f32, "err": err, "bar": bar}


@functools.lru_cache(maxsize=None)
def reference_of(shape, keep=(True, True, True)) -> dict:
    """``reference`` of the case of ``shape`` with the biases of ``keep`` (computed once, shared)."""
    return reference(without_biases(build(shape), keep))


OVER_LIMIT = ((8, 1025, 4, 2), (8, 4, 1025, 2), (8, 4, 4, 65))  # one width past the kernel's limits each: the module's torch path


@functools.lru_cache(maxsize=None)
def over_limit_case(shape) -> dict:
    """The recipe of ``case`` at a width the kernel refuses (no kink condition: only the logits are compared, and ReLU is continuous)."""
    F, H1, H2, C = shape
    gen = torch.Generator().manual_seed(3)
    n = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    c = {"y": n(F), "w1": n(H1, F) / F ** 0.5, "b1": 0.1 * n(H1), "w2": n(H2, H1) / H1 ** 0.5, "b2": 0.1 * n(H2),
         "w3": n(C, H2) / H2 ** 0.5, "b3": 0.1 * n(C), "g": n(C)}
    return {k: v.float().double() for k, v in c.items()}


ANY_ORDER_SIGMAS = 6.0


def any_order_logits_bound(c: dict) -> torch.Tensor:
    """Per logit, how far fp32 arithmetic strays from float64 whatever the order of its sums (the torch path's GEMV is not ours to
    know).  In a dot product of n terms plus a bias every term passes through at most n + 1 roundings, each a relative error
    of at most u = 2^-24; taken as independent they give the result a variance of at most (n + 1) u^2 (sum_k (w_k h_k)^2 + b^2),
    in any order, fused or not.  An input error of variance s_k^2 adds sum_k w_k^2 s_k^2 (the ReLU passes at most what it gets).
    The bound is ANY_ORDER_SIGMAS standard deviations: a few 1e-5 of the logits, the bar of a routing check - the kernels' own
    bars (``reference``) are ten times tighter.  (The worst-case bound, gamma_n |w| . |h| through three layers, is 1e-2: no bar.)"""
    u = 2.0 ** -24
    var = torch.zeros_like(c["y"])
    exact = evaluate(c)
    for k, h in ((1, c["y"]), (2, exact["h1"]), (3, exact["h2"])):
        w, b = c[f"w{k}"], c[f"b{k}"]
        own = (w * w) @ (h * h) + (b * b if b is not None else 0.0)
        var = (w * w) @ var + (w.size(1) + 1) * u * u * own
    return ANY_ORDER_SIGMAS * var.sqrt()


EDGE_UNITS = {3: 0.0, 17: -0.0, 40: -0.5, 64: 0.0}  # fc1 unit -> its pre-activation (row of w1 zeroed, b1 set to this)


@functools.lru_cache(maxsize=None)
def relu_edge_case() -> dict:
    """BIAS_SHAPE's case with the fc1 units of EDGE_UNITS at a pre-activation of exactly 0.0, -0.0 or a negative value."""
    c = {k: v.clone() for k, v in build(BIAS_SHAPE).items()}
    for k, v in EDGE_UNITS.items():
        c["w1"][k].zero_()
        c["b1"][k] = v
    z1, _, z2, _, _ = forward64(*(c[k] for k in INPUTS[:7]))
    others = torch.ones_like(z1, dtype=torch.bool)
    others[list(EDGE_UNITS)] = False
    assert kink_ratio(z1[others]) >= KINK and kink_ratio(z2) >= KINK  # the units not placed on the kink keep their distance
    return c


if __name__ == "__main__":
    for s in SHAPES:
        r, c = reference_of(s), build(s)
        z = evaluate(c)
        print(f"{case_id(s):>18} seed {SEEDS[s]} kink {kink_ratio(z['z1']):.1e} {kink_ratio(z['z2']):.1e}  " + "  ".join(
            f"{k} {r['err'][k] / max(float(r['ref'][k].abs().max()), 1e-300):.1e}" for k in OUTPUTS + GRADS))
