#!/usr/bin/env python3
"""Batch norm over table rows: the K14 route (csrc/batchnorm.hip) beside PyTorch-ROCm's ``F.batch_norm(...) + residual`` and its
autograd, in the same process on the same device, alternating the two.

    python tools/profile_batchnorm.py [--iters 30] [--warmup 5] [--out profiles/batchnorm.txt]

Times with HIP events: forward = statistics + normalise + residual (running statistics updated), backward = the gradients of
z, gamma, beta (the residual's gradient is grad_out).  Algorithmic bytes: 4 passes of 4 * rows * C forward (read z; read z,
read residual, write out), 5 backward (read grad_out, z; read grad_out, z, write dz); the fraction is of 8 TB/s.
Needs a GPU: there is no fallback."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((10_000_000, 64), (1_500_000, 128), (1984, 128))
PEAK_BYTES_PER_S = 8.0e12


def timed(fn, iters):
    """Median and minimum milliseconds of ``fn`` over ``iters`` event-timed calls."""
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_batchnorm: needs a GPU")
    from graphnet_classifier_amd import functional as Fn, native
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    lines = [f"device {torch.cuda.get_device_name(0)}, {a.iters} timed calls after {a.warmup} warm-up calls each, HIP events, ms = median (min)"]
    for rows, width in SHAPES:
        g = torch.Generator(device=dev).manual_seed(rows + width)
        z = torch.randn(rows, width, device=dev, generator=g).requires_grad_(True)
        res = torch.randn(rows, width, device=dev, generator=g)
        grad = torch.randn(rows, width, device=dev, generator=g)
        gamma = (0.5 + torch.rand(width, device=dev, generator=g)).requires_grad_(True)
        beta = torch.rand(width, device=dev, generator=g).requires_grad_(True)
        rm, rv = torch.zeros(width, device=dev), torch.ones(width, device=dev)
        routes = {
            "K14": lambda: Fn.batch_norm_rows(z, gamma, beta, res, rm, rv, 0.1, 1e-5, True),
            "torch": lambda: F.batch_norm(z, rm, rv, gamma, beta, True, 0.1, 1e-5) + res,
        }
        outs = {k: f() for k, f in routes.items()}
        grads = {k: torch.autograd.grad(o, [z, gamma, beta], grad, retain_graph=True) for k, o in outs.items()}
        diff = float((outs["K14"] - outs["torch"]).abs().max())
        gdiff = max(float((p - q).abs().max()) for p, q in zip(grads["K14"], grads["torch"]))
        timers = native.KernelTimers()
        native.set_kernel_timers(timers)
        torch.autograd.grad(routes["K14"](), [z, gamma, beta], grad)
        native.set_kernel_timers(None)
        # above the one-launch kernels' row limit: + the finalize and the partial-sum reduction, which are not timed by name
        launches = timers.num_launches() + (2 if rows > native.bn_small_max_rows() else 0)
        res_ms = {}
        for _ in range(a.warmup):
            for k in routes:
                torch.autograd.grad(routes[k](), [z, gamma, beta], grad)
        for k in ("K14", "torch", "K14", "torch"):  # alternate the two routes; keep the better median of each
            fwd = timed(routes[k], a.iters)
            out = routes[k]()
            bwd = timed(lambda: torch.autograd.grad(out, [z, gamma, beta], grad, retain_graph=True), a.iters)
            if k not in res_ms or fwd[0] + bwd[0] < res_ms[k][0][0] + res_ms[k][1][0]:
                res_ms[k] = (fwd, bwd)
        nbytes = 4.0 * rows * width
        lines.append(f"[{rows}, {width}]  max |out diff| {diff:.2e}, max |grad diff| {gdiff:.2e}, K14 launches forward + backward: {launches}")
        for k in ("K14", "torch"):
            (fm, fmin), (bm, bmin) = res_ms[k]
            lines.append(f"  {k:5s} forward {fm:8.4f} ({fmin:8.4f}) ms = {4 * nbytes / (fm * 1e-3) / PEAK_BYTES_PER_S:6.1%} of 8 TB/s   "
                         f"backward {bm:8.4f} ({bmin:8.4f}) ms = {5 * nbytes / (bm * 1e-3) / PEAK_BYTES_PER_S:6.1%} of 8 TB/s")
        del outs, grads, out
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
