#!/usr/bin/env python3
"""K21 (attention neighbourhood aggregation) forward and backward beside the same math in torch ops and beside K18 MEAN on the same
rows, on one device.

Shapes: the large table of the aggregation benchmarks - N = 1 M destinations, E = 10 M rows, D = 64, destinations drawn uniformly
(in-degrees around 10), rows in destination-sorted order as the model holds them - and one 1,000-node graph (E = 6,000, D = 128).

Sides, forward: ``native.segment_softmax_csr`` (K21); ``native.segment_reduce_csr(..., "mean")`` (K18) on the same rows; torch:
``scatter_reduce(amax)``, ``exp``, two ``index_add_`` and a division.  Backward: ``native.segment_softmax_backward``; K18's
``segment_reduce_backward`` (mean); torch: the closed form of the two gradients with index gathers and a row sum.

Bytes are algorithmic: forward ``4 D E + 8 E + 4 D N + 8 N + 4 (N + 1)`` - the rows once, the scores twice, the
output and (m, Z) once, the row pointers -; K18 MEAN moves the same without the ``8 E`` of scores and the ``8 N`` of (m, Z).  The
expectation the ratio is held against: K21's forward streams K18 MEAN's rows plus 8 E bytes of scores.

Timing: every side warmed up, then ``rounds`` rounds in which windows of ``iters`` calls of the sides alternate; a window is ONE
pair of HIP events with a synchronise behind it.  Median / min / max over rounds, ms per call.  Results go to
``profiles/attention_aggregation.json``.

    python tools/bench_attention_aggregation.py [rounds=7] [iters=10] [out=profiles/attention_aggregation.json]"""
import datetime
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import native  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "attention_aggregation.json")
DEV = torch.device("cuda:0")
SHAPES = (("N = 1 M, E = 10 M, D = 64", 1_000_000, 10_000_000, 64), ("N = 1,000, E = 6,000, D = 128", 1_000, 6_000, 128))


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def alternate(sides, iters, rounds):
    """{name: {"median", "min", "max"}} in ms per call; the sides' windows alternate, so all see the same machine state."""
    for fn in sides.values():
        window(fn, 3)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(window(fn, iters))
    return {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()}


def torch_forward(x, s, dst, n):
    m = torch.full((n,), float("-inf"), device=x.device).scatter_reduce(0, dst, s, "amax")
    e = torch.exp(s - m[dst])
    z = torch.zeros(n, device=x.device).index_add_(0, dst, e)
    num = torch.zeros(n, x.size(1), device=x.device).index_add_(0, dst, e[:, None] * x)
    return torch.where(z[:, None] > 0, num / z[:, None], torch.zeros((), device=x.device)), m, z


def torch_backward(grad, x, s, out, m, z, dst):
    alpha = torch.exp(s - m[dst]) / z[dst]
    g = grad[dst]
    return alpha[:, None] * g, alpha * (g * (x - out[dst])).sum(1)


def one_shape(name, n, e, d):
    gen = torch.Generator(device=DEV).manual_seed(21)
    dst = torch.sort(torch.randint(0, n, (e,), device=DEV, generator=gen)).values
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(torch.bincount(dst, minlength=n), 0)]).int()
    dst32 = dst.int()
    x = torch.randn(e, d, device=DEV, generator=gen)
    s = torch.randn(e, device=DEV, generator=gen) * 3
    grad = torch.randn(n, d, device=DEV, generator=gen)
    out, saved = native.segment_softmax_csr(x, s, rowptr, None, n)
    t_out, t_m, t_z = torch_forward(x, s, dst, n)
    g_src, g_s = native.segment_softmax_backward(grad, x, s, out, saved, dst32)
    t_src, t_s = torch_backward(grad, x, s, t_out, t_m, t_z, dst)
    diffs = {"forward": float((out - t_out).abs().max()), "grad_src": float((g_src - t_src).abs().max()),
             "grad_scores": float((g_s - t_s).abs().max())}
    del t_src, t_s, g_src, g_s
    iters = ITERS if e >= 1_000_000 else 100 * ITERS  # the small graph: enough calls per window to measure more than the clock
    fwd = alternate({"k21": lambda: native.segment_softmax_csr(x, s, rowptr, None, n),
                     "k18_mean": lambda: native.segment_reduce_csr(x, rowptr, None, n, "mean"),
                     "torch": lambda: torch_forward(x, s, dst, n)}, iters, ROUNDS)
    bwd = alternate({"k21": lambda: native.segment_softmax_backward(grad, x, s, out, saved, dst32),
                     "k18_mean": lambda: native.segment_reduce_backward(grad, dst32, rowptr, None, "mean"),
                     "torch": lambda: torch_backward(grad, x, s, t_out, t_m, t_z, dst)}, iters, ROUNDS)
    k21_bytes = 4 * d * e + 8 * e + 4 * d * n + 8 * n + 4 * (n + 1)
    k18_bytes = 4 * d * e + 4 * d * n + 4 * (n + 1)
    bwd_bytes = 8 * d * e + 12 * e + 8 * d * n + 8 * n  # src read, grad_src written; scores, dst, grad_scores; grad_out, out; saved
    f, b = fwd["k21"]["median"], bwd["k21"]["median"]
    entry = {"shape": name, "nodes": n, "rows": e, "width": d, "max_abs_vs_torch": diffs, "iters": iters, "forward_ms": fwd, "backward_ms": bwd,
             "forward_algorithmic_bytes": k21_bytes, "k18_mean_algorithmic_bytes": k18_bytes, "backward_algorithmic_bytes": bwd_bytes,
             "forward_GBps": k21_bytes / (f * 1e-3) / 1e9, "k18_mean_GBps": k18_bytes / (fwd["k18_mean"]["median"] * 1e-3) / 1e9,
             "backward_GBps": bwd_bytes / (b * 1e-3) / 1e9,
             "forward_over_k18_mean": f / fwd["k18_mean"]["median"], "expected_from_bytes": k21_bytes / k18_bytes,
             "backward_over_k18_mean_backward": b / bwd["k18_mean"]["median"],
             "forward_speedup_vs_torch": fwd["torch"]["median"] / f, "backward_speedup_vs_torch": bwd["torch"]["median"] / b}
    print(f"{name:32s} forward K21 {f * 1e3:9.1f} us ({entry['forward_GBps']:7.1f} GB/s)  K18 mean {fwd['k18_mean']['median'] * 1e3:9.1f} us  "
          f"torch {fwd['torch']['median'] * 1e3:9.1f} us  K21 / K18 {entry['forward_over_k18_mean']:.3f} (bytes: "
          f"{entry['expected_from_bytes']:.3f})", flush=True)
    print(f"{'':32s} backward K21 {b * 1e3:9.1f} us ({entry['backward_GBps']:7.1f} GB/s)  K18 mean {bwd['k18_mean']['median'] * 1e3:9.1f} us  "
          f"torch {bwd['torch']['median'] * 1e3:9.1f} us", flush=True)
    return entry


def main():
    assert torch.cuda.is_available(), "bench_attention_aggregation needs a GPU: there is no CPU timing of a GPU kernel"
    native.load_library()
    props = torch.cuda.get_device_properties(0)
    with torch.no_grad():
        shapes = [one_shape(*shape) for shape in SHAPES]
    doc = {"tool": "tools/bench_attention_aggregation.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", ""), "compute_units": props.multi_processor_count,
           "date": datetime.date.today().isoformat(), "rounds": ROUNDS, "iters": ITERS,
           "timing": "HIP events around windows of `iters` calls, the sides' windows alternating; ms per call, output allocation included",
           "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
