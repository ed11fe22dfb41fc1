#!/usr/bin/env python3
"""Capacity-padded top-K pooling (K20, ``GraphNet(pool_ratio=..., pool_padded=True)``) beside the sized form, on one device.

The sized form shrinks every launch behind a pooling layer and pays one host read-back per layer; the padded form reads nothing
back, so a hipGraph capture can record it, and pays for that with launches over all ``rows`` / E behind every layer (and a scorer
over all rows).  Neither is faster by construction; this tool measures where each one is.

1. Forwards of ``CombinedModel(GraphNet(**graphnet_kwargs(128, 3)), readout="mean")`` on the 128 x 128 pixel graph (16,384 nodes,
   32,512 edges), ratio 0.5 behind every block: un-pooled eager and through ``CapturedForward``; pooled sized, eager; pooled
   padded, eager; pooled padded through ``CapturedForward``.  Eager = ``model((x, pos, edge_index))`` on device tensors (the topology
   comes from the cache); captured = ``capture(x, pos)`` (two input copies and the replay).
2. The training step on a ragged batch of 8 superpixel-sized graphs (``synthetic.superpixel_like_graphs``), width 64, two blocks:
   pooled sized, eager (``forward_batched``, mean cross-entropy, backward, fused Adam; the topology cache is cleared in front of
   every step, as a loader that hands out a new region adjacency per batch leaves it) beside pooled padded through
   ``CapturedRaggedBatchStep`` (the feed launch and the replay, topology build inside).
3. ONE pooling layer, ``functional.topk_pool`` padded beside sized, at the three shapes of tools/bench_topk_pool.py.

Timing: every side warmed up, then ``rounds`` rounds in which windows of ``iters`` calls of the sides alternate; a window lies
between two HIP events and is closed by ONE synchronise (the sized sides synchronise inside every call as well: that is part of what
is measured).  Median / min / max over the rounds, in ms per call.  Before anything is timed, and again behind the timed
forwards, the padded logits are compared with the sized ones.  Results go to ``profiles/topk_pool_padded.json``.

    python tools/bench_topk_pool_padded.py [rounds=9] [iters=100] [out=profiles/topk_pool_padded.json]"""
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_topk_pool import alternate, grid_edges, shapes  # noqa: E402
from graphnet_classifier_amd import functional as Fn  # noqa: E402
from graphnet_classifier_amd import native, synthetic, topology  # noqa: E402
from graphnet_classifier_amd.GNN import CapturedForward, CombinedModel, GraphNet  # noqa: E402
from graphnet_classifier_amd.topology import GraphTopology  # noqa: E402

ROUNDS = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "topk_pool_padded.json")
DEV = torch.device("cuda:0")
RATIO = 0.5


def _model(kwargs, num_nodes, **extra):
    torch.manual_seed(0)  # pool_padded adds no parameter: the sized and the padded model hold the same weights
    return CombinedModel(GraphNet(**kwargs, **extra), num_nodes=num_nodes, classes=2, readout="mean").to(DEV)


def forwards():
    n = 128 * 128
    ei = grid_edges().to(DEV)
    x, pos = torch.rand(n, 3, device=DEV), torch.rand(n, 2, device=DEV)
    kw = synthetic.graphnet_kwargs(128, 3)
    models = {"unpooled": _model(kw, n).eval(), "sized": _model(kw, n, pool_ratio=RATIO).eval(),
              "padded": _model(kw, n, pool_ratio=RATIO, pool_padded=True).eval()}
    with torch.no_grad():  # every model's first forward runs eagerly, in front of its capture
        first = {name: m((x, pos, ei)).clone() for name, m in models.items()}
    captures = {"unpooled": CapturedForward(models["unpooled"], x, pos, ei), "padded": CapturedForward(models["padded"], x, pos, ei)}

    def eager(m):
        def run():
            with torch.no_grad():
                m((x, pos, ei))
        return run

    sides = {"unpooled_eager": eager(models["unpooled"]), "unpooled_captured": lambda: captures["unpooled"](x, pos),
             "pooled_sized_eager": eager(models["sized"]), "pooled_padded_eager": eager(models["padded"]),
             "pooled_padded_captured": lambda: captures["padded"](x, pos)}
    with torch.no_grad():
        want = first["sized"]
        replays = []
        for _ in range(2):
            replays.append(captures["padded"](x, pos).clone())
            torch.cuda.synchronize()
        agree = {"padded_eager_vs_sized": float((first["padded"] - want).abs().max()),
                 "padded_captured_vs_sized": float((replays[0] - want).abs().max()),
                 "unpooled_captured_vs_eager": float((captures["unpooled"](x, pos) - first["unpooled"]).abs().max()),
                 # how far two runs of ONE path lie apart, and how large the logits are: what the figures above are read against
                 "sized_eager_twice": float((models["sized"]((x, pos, ei)) - want).abs().max()),
                 "padded_captured_twice": float((replays[0] - replays[1]).abs().max()),
                 "max_abs_logit": float(want.abs().max())}
    t = alternate(sides, ITERS, ROUNDS)
    with torch.no_grad():  # and behind the timing: what was timed still computes the sized logits
        agree["padded_captured_after_timing_vs_sized"] = float((captures["padded"](x, pos) - want).abs().max())
        agree["unpooled_captured_after_timing_vs_eager"] = float((captures["unpooled"](x, pos) - first["unpooled"]).abs().max())
    for name, v in t.items():
        print(f"forward, 128 x 128 grid, {name:24s} {v['median'] * 1e3:8.1f} us  [{v['min'] * 1e3:.1f}, {v['max'] * 1e3:.1f}]", flush=True)
    print("  max |logits - reference|:", agree, flush=True)
    return {"form": "CombinedModel(GraphNet(**graphnet_kwargs(128, 3)), readout='mean') on the 128 x 128 pixel graph (16,384 nodes, "
                    "32,512 edges), no_grad, inputs on the device; pooled: ratio 0.5 behind every block; eager = model((x, pos, "
                    "edge_index)) with the topology from the cache, captured = CapturedForward(x, pos)",
            "ms": t, "max_abs_logit_difference": agree, "rows_out": models["sized"].graph_net.pooled_nodes(n)}


def ragged_step():
    from graphnet_classifier_amd.train import CapturedRaggedBatchStep, FlatParameters, FusedAdam, padded_capacity
    batch = synthetic.superpixel_like_graphs(8, seed=1000).to(DEV)
    labels = torch.arange(8) % 2
    labels_dev = labels.to(DEV)
    gptr = batch.graph_ptr.to(DEV)
    kw = synthetic.graphnet_kwargs(64, 2)
    crit = torch.nn.CrossEntropyLoss()
    sized, padded = _model(kw, 100, pool_ratio=RATIO), _model(kw, 100, pool_ratio=RATIO, pool_padded=True)
    opt_s, opt_p = FusedAdam(FlatParameters(sized)), FusedAdam(FlatParameters(padded))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    E = padded_capacity(int(batch.edge_index.size(1)))
    N = padded_capacity(int(batch.x.size(0)), 0, 32)
    with torch.no_grad():
        agree = float((padded.forward_batched(batch.x, batch.pos, batch.edge_index, graph_ptr=gptr)
                       - sized.forward_batched(batch.x, batch.pos, batch.edge_index, graph_ptr=gptr)).abs().max())
    step = CapturedRaggedBatchStep(padded, opt_p, crit, batch, labels, loss_sum, edge_capacity=E, node_capacity=N)

    def eager():
        topology._default_cache.clear()  # a new region adjacency per batch: the build (and its read-back) is part of the step
        loss = crit(sized.forward_batched(batch.x, batch.pos, batch.edge_index, graph_ptr=gptr), labels_dev)
        opt_s.zero_grad()
        loss.backward()
        opt_s.step()

    t = alternate({"pooled_sized_eager": eager, "pooled_padded_captured": lambda: step(batch, labels)}, ITERS, ROUNDS)
    step.check()
    for name, v in t.items():
        print(f"ragged batch step, 8 graphs, {name:24s} {v['median'] * 1e3:8.1f} us  [{v['min'] * 1e3:.1f}, {v['max'] * 1e3:.1f}]", flush=True)
    return {"form": "training step of CombinedModel(GraphNet(**graphnet_kwargs(64, 2), pool_ratio=0.5), readout='mean') on a batch of 8 "
                    "superpixel-like graphs; sized: eager forward_batched + mean cross-entropy + backward + fused Adam with a fresh "
                    "topology build per step; padded: CapturedRaggedBatchStep (feed launch + replay, build inside)",
            "nodes": int(batch.x.size(0)), "edges": int(batch.edge_index.size(1)), "node_capacity": N, "edge_capacity": E, "ms": t,
            "max_abs_logit_difference_before_training": agree}


def layers():
    out = []
    for name, sizes, C, ei in shapes():
        rows = int(sizes.sum())
        topo = GraphTopology(ei.to(DEV), rows, device=DEV)
        gp = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(DEV)
        x, s, e = torch.randn(rows, C, device=DEV), torch.randn(rows, device=DEV), torch.randn(topo.num_edges, C, device=DEV)

        def layer(padded):
            def run():
                with torch.no_grad():
                    return Fn.topk_pool(x, s, topo, gp, RATIO, e, padded=padded)
            return run

        a, b = layer(False)(), layer(True)()
        n_out, e_out = a[0].size(0), a[1].size(0)
        same = (torch.equal(b[0][:n_out], a[0]) and torch.equal(b[1][:e_out], a[1]) and torch.equal(b[4][:n_out], a[4])
                and not bool(b[0][n_out:].any()) and int(b[2].rowptr[-1]) == topo.num_edges)
        t = alternate({"sized": layer(False), "padded": layer(True)}, ITERS, ROUNDS)
        print(f"layer, {name:44s} sized {t['sized']['median'] * 1e3:8.1f} us  padded {t['padded']['median'] * 1e3:8.1f} us  "
              f"prefix equal, tail zero: {same}", flush=True)
        out.append({"shape": name, "rows": rows, "edges": topo.num_edges, "width": C, "kept_rows": n_out, "kept_edges": e_out,
                    "padded_prefix_equals_sized": bool(same), "sized_ms": t["sized"], "padded_ms": t["padded"],
                    "padded_over_sized": t["padded"]["median"] / t["sized"]["median"]})
    return out


def main():
    assert torch.cuda.is_available(), "bench_topk_pool_padded needs a GPU: there is no CPU timing of a GPU kernel"
    native.load_library()
    props = torch.cuda.get_device_properties(0)
    doc = {"tool": "tools/bench_topk_pool_padded.py", "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""),
           "compute_units": props.multi_processor_count, "date": datetime.date.today().isoformat(), "rounds": ROUNDS, "iters": ITERS,
           "ratio": RATIO,
           "timing": "HIP events around windows of `iters` calls, the sides' windows alternating; median / min / max over the rounds, "
                     "ms per call, host read-backs included",
           "forwards": forwards(), "ragged_batch_step": ragged_step(), "layers": layers()}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
