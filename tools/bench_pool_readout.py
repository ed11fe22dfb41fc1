#!/usr/bin/env python3
"""K17 (global pooling read-out) against the same pooling written with torch ops on the same device, forward and backward.

Shapes: 10,000 graphs x ~150 rows x C = 128 (c2-like); 64 superpixel graphs x ~100 rows x C = 64; one 16,384-row graph x C = 128
(a 128 x 128 pixel graph, the split regime).  Mode ``hybrid`` (mean | max | sum from one pass), which is what the torch side needs
three reductions for: ``index_add_`` over a row -> graph index for the sum, the division for the mean, ``segment_reduce`` for the
max; its backward is torch autograd's.

Timing: every shape and both sides warmed up, then ``rounds`` rounds in which windows of ``iters`` calls of K17 and of torch
alternate; a window is closed by ONE device synchronise between two HIP events.  Median / min / max over rounds per call.  Bytes
are the algorithmic ones - forward reads y once (``rows * C * 4``; the [G, 3C] outputs and the int32 argmax are added), backward
writes dy once and reads the [G, 3C] gradient and the argmax - and the GB/s column is those over the median time, to be read
against the 5.9 - 6.1 TB/s a pure read stream reaches on the part.  Results go to ``profiles/pool_readout.json``.

    python tools/bench_pool_readout.py [rounds=9] [iters=50] [out=profiles/pool_readout.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import functional as Fn  # noqa: E402
from graphnet_classifier_amd import native  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pool_readout.json")
DEV = torch.device("cuda:0")


def shapes():
    gen = torch.Generator().manual_seed(17)
    many = torch.randint(120, 181, (10_000,), generator=gen)   # ~150 rows
    sp = torch.randint(70, 131, (64,), generator=gen)          # ~100 rows
    return [("10000 graphs x ~150 rows x 128", many, 128), ("64 graphs x ~100 rows x 64", sp, 64),
            ("1 graph x 16384 rows x 128", torch.tensor([16384]), 128)]


def torch_hybrid(y, graph_of, sizes, G):
    """The same read-out with torch ops: sum by index_add_, mean by division, max by segment_reduce."""
    psum = torch.zeros(G, y.size(1), dtype=y.dtype, device=y.device).index_add_(0, graph_of, y)
    pmean = psum / sizes.clamp(min=1).to(y.dtype)[:, None]
    pmax = torch.segment_reduce(y, "max", lengths=sizes, axis=0, unsafe=True)
    return torch.cat([pmean, pmax, psum], dim=1)


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def main():
    assert torch.cuda.is_available(), "bench_pool_readout needs a GPU: there is no CPU timing of a GPU kernel"
    native.load_library()
    results = []
    for name, sizes, C in shapes():
        G, rows = sizes.numel(), int(sizes.sum())
        gp = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(DEV)
        sizes_d = sizes.to(DEV)
        graph_of = torch.repeat_interleave(torch.arange(G, device=DEV), sizes_d)
        y = torch.randn(rows, C, device=DEV)
        grad = torch.randn(G, 3 * C, device=DEV)
        plan = native.graph_pool_plan(rows, C, G)
        modes = native.POOL_MODES["hybrid"]
        out, argmax = native.graph_pool_forward(y, gp, modes)
        ref = torch_hybrid(y, graph_of, sizes_d, G)
        err = float((out - ref).abs().max())
        yt = y.clone().requires_grad_(True)
        reft = torch_hybrid(yt, graph_of, sizes_d, G)

        def torch_bwd():
            yt.grad = None
            reft.backward(grad, retain_graph=True)

        sides = {
            "forward": (lambda: native.graph_pool_forward(y, gp, modes), lambda: torch_hybrid(y, graph_of, sizes_d, G),
                        4 * (rows * C + 3 * G * C + G * C)),
            "backward": (lambda: native.graph_pool_backward(grad, modes, argmax, gp, rows), torch_bwd, 4 * (rows * C + 3 * G * C + G * C)),
        }
        torch_bwd()
        derr = float((native.graph_pool_backward(grad, modes, argmax, gp, rows) - yt.grad).abs().max())
        entry = {"shape": name, "rows": rows, "graphs": G, "width": C, "split": plan["split"], "chunk_rows": plan["chunk_rows"],
                 "max_abs_forward_vs_torch": err, "max_abs_backward_vs_torch": derr}
        for side, (ours, theirs, nbytes) in sides.items():
            for fn in (ours, theirs):
                window(fn, 5)
            t_ours, t_theirs = [], []
            for _ in range(ROUNDS):  # alternating windows: both sides see the same machine state
                t_ours.append(window(ours, ITERS))
                t_theirs.append(window(theirs, ITERS))
            med = statistics.median(t_ours)
            entry[side] = {"k17_ms": {"median": med, "min": min(t_ours), "max": max(t_ours)},
                           "torch_ms": {"median": statistics.median(t_theirs), "min": min(t_theirs), "max": max(t_theirs)},
                           "algorithmic_bytes": nbytes, "k17_GBps": nbytes / (med * 1e-3) / 1e9,
                           "speedup_vs_torch": statistics.median(t_theirs) / med}
            print(f"{name:34s} {side:8s} K17 {med * 1e3:8.1f} us  torch {statistics.median(t_theirs) * 1e3:8.1f} us  "
                  f"{entry[side]['k17_GBps']:8.1f} GB/s  split={plan['split']}", flush=True)
        results.append(entry)
    doc = {"tool": "tools/bench_pool_readout.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "iters": ITERS,
           "timing": "HIP events around windows of `iters` calls, K17 and torch windows alternating; ms per call",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
