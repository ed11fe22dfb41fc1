#!/usr/bin/env python3
"""K20 (top-K node pooling) per pooling layer beside the same pooling composed from torch ops, and the eager GraphNet forward with
and without pooling, on one device.

1. ONE K20 layer - ``functional.topk_pool``: select, edge filter, the read-back of the two sizes, node and edge row compaction -
   beside a torch composition of the same result: two stable ``argsort`` calls for the per-graph order, a rank mask, ``nonzero``
   (its own host synchronisation) for the kept nodes and the kept edges, ``cumsum`` for the new ids, index gathers, ``bincount`` +
   ``cumsum`` for the pooled CSR offsets.  Shapes: 10,000 graphs x ~150 rows x 128 and 64 graphs x ~100 rows x 64 with four
   in-graph in-edges per node, and 1 graph x 16,384 rows x 128 with the 128 x 128 pixel grid's 32,512 edges.  Ratio 0.5.
2. The eager forward of ``GraphNet(**graphnet_kwargs(128, 3))`` on the 128 x 128 pixel graph with ``pool_ratio`` None and 0.5
   (pooling behind every block: blocks 2 and 3 see 8,192 and 4,096 nodes).

Bytes are algorithmic: a layer reads the scores (4 passes of the radix select and the final walk are L2 hits after the first),
reads E (src, dst) pairs twice and writes at most 4 int32 per edge, and moves the kept rows once: ``4 (rows + 2 N' C + 2 E' De) +
4 (4 E + 4 E')`` bytes.

Timing: every side warmed up, then ``rounds`` rounds in which windows of ``iters`` calls of the sides alternate; a window is closed
by ONE device synchronise between two HIP events (every call of either side synchronises inside as well: that is part of what is
measured).  Median / min / max over rounds per call.  Results go to ``profiles/topk_pool.json``.

    python tools/bench_topk_pool.py [rounds=9] [iters=20] [out=profiles/topk_pool.json]"""
import datetime
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import functional as Fn  # noqa: E402
from graphnet_classifier_amd import native  # noqa: E402
from graphnet_classifier_amd.topology import GraphTopology  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "topk_pool.json")
DEV = torch.device("cuda:0")
RATIO = 0.5


def grid_edges():
    from oracle import graphnet_oracle as O
    return torch.from_numpy(O.grid_edge_index(128, 128))


def shapes():
    gen = torch.Generator().manual_seed(17)
    many = torch.randint(120, 181, (10_000,), generator=gen)   # ~150 rows
    sp = torch.randint(70, 131, (64,), generator=gen)          # ~100 rows
    out = []
    for name, sizes, C in (("10000 graphs x ~150 rows x 128", many, 128), ("64 graphs x ~100 rows x 64", sp, 64)):
        rows = int(sizes.sum())
        start = torch.repeat_interleave(torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)[:-1]]), sizes)
        size_of = torch.repeat_interleave(sizes, sizes)
        dst = torch.arange(rows).repeat_interleave(4)
        src = start[dst] + torch.minimum((torch.rand(4 * rows, generator=gen) * size_of[dst]).long(), size_of[dst] - 1)
        out.append((name, sizes, C, torch.stack([src, dst])))
    out.append(("1 graph x 16384 rows x 128, 128 x 128 grid", torch.tensor([16384]), 128, grid_edges()))
    return out


def torch_topk(x, s, e, src, dst, graph_of, gp, k_of_graph):
    """The same pooling layer with torch ops (two host synchronisations: the two ``nonzero`` calls)."""
    rows = x.size(0)
    order = torch.argsort(s, descending=True, stable=True)
    order = order[torch.argsort(graph_of[order], stable=True)]
    g_sorted = graph_of[order]
    keep_sorted = torch.arange(rows, device=x.device) - gp[g_sorted] < k_of_graph[g_sorted]
    mask = torch.zeros(rows, dtype=torch.bool, device=x.device)
    mask[order] = keep_sorted
    kept = mask.nonzero().view(-1)
    new_id = torch.cumsum(mask, 0) - 1
    x2 = x[kept] * torch.tanh(s[kept])[:, None]
    kept_edges = (mask[src] & mask[dst]).nonzero().view(-1)
    src2, dst2, e2 = new_id[src[kept_edges]], new_id[dst[kept_edges]], e[kept_edges]
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(torch.bincount(dst2, minlength=kept.numel()), 0)])
    gp2 = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(k_of_graph, 0)])
    return x2, e2, src2, dst2, rowptr, gp2, kept


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


def layers():
    results = []
    for name, sizes, C, ei in shapes():
        G, rows, De = sizes.numel(), int(sizes.sum()), C
        topo = GraphTopology(ei.to(DEV), rows, device=DEV)
        E = topo.num_edges
        gp = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(DEV)
        graph_of = torch.repeat_interleave(torch.arange(G, device=DEV), sizes.to(DEV))
        k_of_graph = torch.tensor([native.topk_keep_count(RATIO, int(n)) for n in sizes.tolist()], device=DEV)
        x, s, e = torch.randn(rows, C, device=DEV), torch.randn(rows, device=DEV), torch.randn(E, De, device=DEV)
        src64, dst64 = topo.src_sorted.long(), topo.dst_sorted.long()
        with torch.no_grad():
            x2, e2, topo2, gp2, kept = Fn.topk_pool(x, s, topo, gp, RATIO, e)
            tx, te, tsrc, tdst, trp, tgp, tkept = torch_topk(x, s, e, src64, dst64, graph_of, gp, k_of_graph)
        same = (torch.equal(kept.long(), tkept) and torch.equal(topo2.src_sorted.long(), tsrc) and torch.equal(topo2.dst_sorted.long(), tdst)
                and torch.equal(topo2.rowptr.long(), trp) and torch.equal(gp2, tgp) and torch.equal(e2, te))
        n_out, e_out = kept.numel(), topo2.num_edges
        nbytes = 4 * (rows + 2 * n_out * C + 2 * e_out * De) + 4 * (4 * E + 4 * e_out)

        def k20():
            with torch.no_grad():
                Fn.topk_pool(x, s, topo, gp, RATIO, e)

        def composed():
            with torch.no_grad():
                torch_topk(x, s, e, src64, dst64, graph_of, gp, k_of_graph)

        t = alternate({"k20": k20, "torch": composed}, ITERS, ROUNDS)
        med = t["k20"]["median"]
        entry = {"shape": name, "rows": rows, "graphs": G, "width": C, "edges": E, "kept_rows": n_out, "kept_edges": e_out,
                 "same_integers_as_torch": bool(same), "max_abs_rows_vs_torch": float((x2 - tx).abs().max()), "k20_ms": t["k20"],
                 "torch_ms": t["torch"], "algorithmic_bytes": nbytes, "k20_GBps": nbytes / (med * 1e-3) / 1e9,
                 "speedup_vs_torch": t["torch"]["median"] / med}
        print(f"{name:44s} K20 {med * 1e3:9.1f} us  torch {t['torch']['median'] * 1e3:9.1f} us  x{entry['speedup_vs_torch']:.2f}  "
              f"{entry['k20_GBps']:7.1f} GB/s  same integers: {same}", flush=True)
        results.append(entry)
    return results


def eager_forward():
    """ms per eager GraphNet forward on the 128 x 128 pixel graph, pool_ratio None beside 0.5."""
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import GraphNet
    ei = grid_edges().to(DEV)
    n = 128 * 128
    x, pos = torch.rand(n, 3, device=DEV), torch.rand(n, 2, device=DEV)
    topo = GraphTopology(ei, n, device=DEV)
    sides, keep = {}, []
    for label, extra in (("unpooled", {}), ("pooled", {"pool_ratio": RATIO})):
        torch.manual_seed(0)
        m = GraphNet(**synthetic.graphnet_kwargs(128, 3), **extra).to(DEV).eval()
        keep.append(m)

        def run(m=m):
            with torch.no_grad():
                m.forward_device(x, pos, topo)
        sides[label] = run
    t = alternate(sides, ITERS, ROUNDS)
    rows_out = keep[1].pooled_nodes(n)
    print(f"eager forward, 128 x 128 grid, graphnet_kwargs(128, 3): un-pooled {t['unpooled']['median'] * 1e3:.1f} us, pool_ratio 0.5 "
          f"{t['pooled']['median'] * 1e3:.1f} us ({rows_out} rows out)", flush=True)
    return {"form": "GraphNet(**graphnet_kwargs(128, 3)).forward_device on the 128 x 128 pixel graph (16,384 nodes, 32,512 edges), "
                    "no_grad, inputs and topology on the device; pooled: pool_ratio=0.5 behind every block (three read-backs)",
            "unpooled_ms": t["unpooled"], "pooled_ms": t["pooled"], "rows_out": rows_out,
            "pooled_over_unpooled": t["pooled"]["median"] / t["unpooled"]["median"]}


def main():
    assert torch.cuda.is_available(), "bench_topk_pool needs a GPU: there is no CPU timing of a GPU kernel"
    native.load_library()
    props = torch.cuda.get_device_properties(0)
    doc = {"tool": "tools/bench_topk_pool.py", "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""),
           "compute_units": props.multi_processor_count, "date": datetime.date.today().isoformat(), "rounds": ROUNDS, "iters": ITERS,
           "ratio": RATIO,
           "timing": "HIP events around windows of `iters` calls, the sides' windows alternating; ms per call, host read-backs included",
           "layers": layers(), "eager_forward": eager_forward()}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
