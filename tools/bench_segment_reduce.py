#!/usr/bin/env python3
"""K18 (mean / max neighbourhood aggregation) beside K1 (the sum, the unchanged kernel) on the same inputs, forward and backward,
and the c3 forward end to end with ``aggregation="mean"`` / ``"max"`` against ``"sum"``.

Shapes: c3 (N = 1 M destinations, E = 10 M CSR-ordered message rows, D = 64; the chunk kernels) and one 128 x 128 pixel graph with
its 8-neighbourhood at D = 128 (N = 16384: one lane group per destination).
Forward: K1 sum | K18 mean | K18 max without argmax | K18 max with argmax | K1 sum + rows_div_degree (the model's mean route).
Backward: gather_rows (the sum's backward) | K18 mean backward | K18 max backward.

Timing: every variant warmed up, then ``rounds`` rounds in which windows of ``iters`` calls of the variants alternate; a window is
closed by ONE device synchronise between two HIP events.  Median / min / max over rounds per call.  Bytes are the algorithmic ones
(forward: messages once, output once, row pointers, plus the int32 winners when stored; backward: grad_src written once, the
[N, D] gradient - and the winners - read once, one int32 per row) and the GB/s column is those over the median time, to be read
against the 5.9 - 6.1 TB/s a pure read stream reaches on the part.  Results go to ``profiles/segment_reduce.json``.

    python tools/bench_segment_reduce.py [rounds=7] [iters=20] [out=profiles/segment_reduce.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import native, synthetic  # noqa: E402
from graphnet_classifier_amd.GNN import GraphNet  # noqa: E402
from graphnet_classifier_amd.topology import GraphTopology  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "segment_reduce.json")
DEV = torch.device("cuda:0")


def pixel_edges(h: int, w: int) -> torch.Tensor:
    """[2, E] int64: every pixel to its 8 neighbours inside the image."""
    r, c = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    src, dst = [], []
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            ok = (r + dr >= 0) & (r + dr < h) & (c + dc >= 0) & (c + dc < w)
            src.append((r * w + c)[ok])
            dst.append(((r + dr) * w + c + dc)[ok])
    return torch.stack([torch.cat(src), torch.cat(dst)])


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def alternate(variants, iters):
    """{name: {median, min, max} ms per call}: warm-up, then ROUNDS rounds of one window per variant in turn."""
    for fn in variants.values():
        window(fn, 3)
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}


def kernel_level(name, topo, d):
    n, e = topo.num_nodes, topo.num_edges
    msgs = torch.randn(e, d, device=DEV)
    grad = torch.randn(n, d, device=DEV)
    rowptr, dst = topo.rowptr, topo.dst_sorted
    _, argmax = native.segment_reduce_csr(msgs, rowptr, None, n, "max", with_argmax=True)
    sums = torch.empty(n, d, device=DEV)
    base = 4.0 * d * e + 4.0 * d * n + 4.0 * (n + 1)

    def sum_then_divide():
        native.scatter_sum_csr(msgs, rowptr, None, n, out=sums)
        native.rows_div_degree_(sums, rowptr)

    fwd = {"k1_sum": (lambda: native.scatter_sum_csr(msgs, rowptr, None, n, out=sums), base),
           "k18_mean": (lambda: native.segment_reduce_csr(msgs, rowptr, None, n, "mean"), base),
           "k18_max": (lambda: native.segment_reduce_csr(msgs, rowptr, None, n, "max"), base),
           "k18_max_argmax": (lambda: native.segment_reduce_csr(msgs, rowptr, None, n, "max", with_argmax=True), base + 4.0 * d * n),
           "k1_sum_then_div_degree": (sum_then_divide, base + 8.0 * d * n + 4.0 * (n + 1))}
    bwd_base = 4.0 * d * e + 4.0 * e + 4.0 * d * n
    bwd = {"gather_rows_sum_backward": (lambda: native.gather_rows(grad, dst), bwd_base),
           "k18_mean_backward": (lambda: native.segment_reduce_backward(grad, dst, rowptr, None, "mean"), bwd_base + 4.0 * (n + 1)),
           "k18_max_backward": (lambda: native.segment_reduce_backward(grad, dst, rowptr, argmax, "max"), bwd_base + 4.0 * d * n)}
    entry = {"shape": name, "nodes": n, "edges": e, "width": d, "regime": "small" if n <= 64 * torch.cuda.get_device_properties(0).multi_processor_count else "chunk"}
    for side, variants in (("forward", fwd), ("backward", bwd)):
        t = alternate({k: v[0] for k, v in variants.items()}, ITERS)
        entry[side] = {}
        for k, (_, nbytes) in variants.items():
            entry[side][k] = {"ms": t[k], "algorithmic_bytes": nbytes, "GBps": nbytes / (t[k]["median"] * 1e-3) / 1e9}
            print(f"{name:28s} {side:8s} {k:26s} {t[k]['median'] * 1e3:9.1f} us  {entry[side][k]['GBps']:8.1f} GB/s", flush=True)
    return entry


def end_to_end(batch, kwargs, topo):
    x, pos = batch.x.to(DEV), batch.pos.to(DEV)
    models = {}
    for mode in ("sum", "mean", "max"):
        torch.manual_seed(0)
        models[mode] = GraphNet(**kwargs, aggregation=mode).to(DEV).eval()

    def run(m):
        with torch.no_grad():
            m.forward_device(x, pos, topo)

    t = alternate({mode: (lambda m=m: run(m)) for mode, m in models.items()}, max(2, ITERS // 4))
    for mode, v in t.items():
        print(f"c3 forward, aggregation={mode:5s} {v['median']:8.3f} ms ({v['median'] / t['sum']['median']:.3f} x sum)", flush=True)
    return {mode: {"ms": v, "relative_to_sum": v["median"] / t["sum"]["median"]} for mode, v in t.items()}


def main():
    assert torch.cuda.is_available(), "bench_segment_reduce needs a GPU: there is no CPU timing of a GPU kernel"
    native.load_library()
    results = []
    ei = pixel_edges(128, 128).to(DEV)
    results.append(kernel_level("128 x 128 pixel graph", GraphTopology(ei, 128 * 128, device=DEV), 128))
    batch, kwargs = synthetic.make_workload("c3")
    topo = GraphTopology(batch.edge_index.to(DEV), batch.num_nodes, device=DEV)
    results.append(kernel_level("c3: 1M nodes / 10M edges", topo, 64))
    e2e = end_to_end(batch, kwargs, topo)
    doc = {"tool": "tools/bench_segment_reduce.py", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "iters": ITERS,
           "timing": "HIP events around windows of `iters` calls, the variants' windows alternating; ms per call",
           "results": results, "c3_forward_end_to_end": e2e}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
