#!/usr/bin/env python3
"""K19 (attention read-out) per launch, forward and backward, beside two yardsticks on the same device:

1. the same pooling composed from torch ops - ``scatter_reduce_("amax")`` for the per-graph maximum, ``exp``, ``index_add_`` for Z and
   for the weighted column sums, a division - and autograd's backward of that composition;
2. K17 ``hybrid`` (mean | max | sum from one pass) on the same ``y``: it reads the same rows once, so it is the natural yardstick for
   a read-out that is expected to be HBM-bound.

Shapes: those of K17's table in DESIGN.md - 10,000 graphs x ~150 rows x C = 128; 64 superpixel graphs x ~100 rows x C = 64; one
16,384-row graph x C = 128 (the split regime).  Bytes are algorithmic: the forward reads ``rows (C + 1)`` floats once (and writes
[G, C]), the backward reads ``rows (C + 1)`` and writes ``rows (C + 1)``.

Then ONE captured single-graph training step (``CapturedTrainStep(edge_capacity=1024, node_capacity=128)``) of ``readout="attention"``
beside ``readout="mean"`` over the superpixel fixture graphs of tests/golden (69 / 119 / 100 nodes): the difference is the gate MLP
plus K19.

Timing: every shape and side warmed up, then ``rounds`` rounds in which windows of ``iters`` calls of the sides alternate; a window is
closed by ONE device synchronise between two HIP events.  Median / min / max over rounds per call.  Results go to
``profiles/attention_readout.json``.

    python tools/bench_attention_readout.py [rounds=9] [iters=50] [out=profiles/attention_readout.json]"""
import datetime
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import native  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "attention_readout.json")
DEV = torch.device("cuda:0")


def shapes():
    gen = torch.Generator().manual_seed(17)
    many = torch.randint(120, 181, (10_000,), generator=gen)   # ~150 rows
    sp = torch.randint(70, 131, (64,), generator=gen)          # ~100 rows
    return [("10000 graphs x ~150 rows x 128", many, 128), ("64 graphs x ~100 rows x 64", sp, 64),
            ("1 graph x 16384 rows x 128", torch.tensor([16384]), 128)]


def torch_attention(y, s, graph_of, G):
    """The same read-out with torch ops."""
    m = torch.full((G,), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce_(0, graph_of, s.detach(), "amax")
    e = torch.exp(s - m[graph_of])
    Z = torch.zeros(G, dtype=s.dtype, device=s.device).index_add_(0, graph_of, e)
    num = torch.zeros(G, y.size(1), dtype=y.dtype, device=y.device).index_add_(0, graph_of, e[:, None] * y)
    return num / Z[:, None]


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
        window(fn, 5)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(window(fn, iters))
    return {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()}


def kernels():
    results = []
    for name, sizes, C in shapes():
        G, rows = sizes.numel(), int(sizes.sum())
        gp = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(DEV)
        graph_of = torch.repeat_interleave(torch.arange(G, device=DEV), sizes.to(DEV))
        y, s = torch.randn(rows, C, device=DEV), 4 * torch.randn(rows, device=DEV)
        grad, grad3 = torch.randn(G, C, device=DEV), torch.randn(G, 3 * C, device=DEV)
        plan = native.graph_pool_plan(rows, C, G)
        hybrid = native.POOL_MODES["hybrid"]
        out, saved = native.graph_attention_pool_forward(y, s, gp)
        _, argmax = native.graph_pool_forward(y, gp, hybrid)
        yt, st = y.clone().requires_grad_(True), s.clone().requires_grad_(True)
        reft = torch_attention(yt, st, graph_of, G)
        err = float((out - reft.detach()).abs().max())

        def torch_bwd():
            yt.grad = st.grad = None
            reft.backward(grad, retain_graph=True)

        torch_bwd()
        dy, ds = native.graph_attention_pool_backward(grad, y, s, out, saved, gp)
        derr = (float((dy - yt.grad).abs().max()), float((ds - st.grad).abs().max()))
        fwd_bytes, bwd_bytes = 4 * (rows * (C + 1) + G * C), 4 * (2 * rows * (C + 1) + 2 * G * C)
        entry = {"shape": name, "rows": rows, "graphs": G, "width": C, "split": plan["split"], "chunk_rows": plan["chunk_rows"],
                 "max_abs_forward_vs_torch": err, "max_abs_dy_vs_torch": derr[0], "max_abs_ds_vs_torch": derr[1]}
        fwd = alternate({"k19": lambda: native.graph_attention_pool_forward(y, s, gp),
                         "torch": lambda: torch_attention(y, s, graph_of, G),
                         "k17_hybrid": lambda: native.graph_pool_forward(y, gp, hybrid)}, ITERS, ROUNDS)
        bwd = alternate({"k19": lambda: native.graph_attention_pool_backward(grad, y, s, out, saved, gp),
                         "torch": torch_bwd,
                         "k17_hybrid": lambda: native.graph_pool_backward(grad3, hybrid, argmax, gp, rows)}, ITERS, ROUNDS)
        for side, t, nbytes in (("forward", fwd, fwd_bytes), ("backward", bwd, bwd_bytes)):
            med = t["k19"]["median"]
            entry[side] = {"k19_ms": t["k19"], "torch_ms": t["torch"], "k17_hybrid_ms": t["k17_hybrid"], "algorithmic_bytes": nbytes,
                           "k19_GBps": nbytes / (med * 1e-3) / 1e9, "speedup_vs_torch": t["torch"]["median"] / med,
                           "time_over_k17_hybrid": med / t["k17_hybrid"]["median"]}
            print(f"{name:34s} {side:8s} K19 {med * 1e3:8.1f} us  torch {t['torch']['median'] * 1e3:8.1f} us  K17 hybrid "
                  f"{t['k17_hybrid']['median'] * 1e3:8.1f} us  {entry[side]['k19_GBps']:8.1f} GB/s  split={plan['split']}", flush=True)
        results.append(entry)
    return results


def captured_steps():
    """ms per captured single-graph training step, attention beside mean, over the fixture graphs."""
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import CapturedTrainStep, FlatParameters, FusedAdam
    from oracle import image_graph_oracle as IO
    from tests.test_superpixel_golden import CASES
    graphs = []
    for case_id in (20, 10, 35):  # 69 / 119 / 100 nodes
        _, img, labels, _, graph = CASES[case_id]
        graph = graph if graph is not None else IO.superpixel_graph_from_labels(img, labels)
        x, pos, ei = (torch.from_numpy(np.ascontiguousarray(np.asarray(a))) for a in graph)
        graphs.append((x.float().to(DEV), pos.float().to(DEV), ei.long().to(DEV)))
    label = torch.tensor(1, device=DEV)
    sides, keep = {}, []
    for readout in ("attention", "mean"):
        torch.manual_seed(1234)
        m = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(64, 2, out_channels=8)), num_nodes=100, classes=2, readout=readout)
        opt = FusedAdam(FlatParameters(m))
        loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
        step = CapturedTrainStep(m, opt, torch.nn.CrossEntropyLoss(), graphs[1], label, loss_sum, edge_capacity=1024, node_capacity=128)
        keep.append((m, opt, loss_sum, step))

        def run(step=step):
            for g in graphs:
                step(g, label)
        sides[readout] = run
    t = alternate(sides, max(ITERS // 3, 1), ROUNDS)
    per_step = {name: {k: v / len(graphs) for k, v in stats.items()} for name, stats in t.items()}
    print(f"captured single-graph step (node_capacity form, 69 / 119 / 100 nodes): attention "
          f"{per_step['attention']['median'] * 1e3:.1f} us, mean {per_step['mean']['median'] * 1e3:.1f} us", flush=True)
    return {"form": "CapturedTrainStep(edge_capacity=1024, node_capacity=128), graphnet_kwargs(64, 2, out_channels=8), fixture graphs "
                    "of 69 / 119 / 100 nodes in turn; ms per step, inputs already on the device",
            "attention_ms": per_step["attention"], "mean_ms": per_step["mean"],
            "difference_us": (per_step["attention"]["median"] - per_step["mean"]["median"]) * 1e3}


def main():
    assert torch.cuda.is_available(), "bench_attention_readout needs a GPU: there is no CPU timing of a GPU kernel"
    native.load_library()
    doc = {"tool": "tools/bench_attention_readout.py", "device": torch.cuda.get_device_name(0),
           "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "date": datetime.date.today().isoformat(), "rounds": ROUNDS, "iters": ITERS,
           "timing": "HIP events around windows of `iters` calls, the sides' windows alternating; ms per call",
           "results": kernels(), "captured_step": captured_steps()}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
