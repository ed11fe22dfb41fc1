#!/usr/bin/env python3
"""Time per mini-batch of a training step over RAGGED batches: a stream of different batches of 8 superpixel-like graphs
(``synthetic.superpixel_like_graphs(8, seed)``: 144 / 156 / 169 nodes per graph, another adjacency in every batch), device tensors
in as ``GraphImageFolder.loader(batch_size=8)`` yields them, default GraphNet (D = 128) with 3 blocks, ``ragged_readout``.

  eager     the training loop's step with ``capture=False``: topology build with its host read-back, ~150 launches
  captured  the same loop with capture on: one feed launch (gnc_pad_graph_batch) + one hipGraph replay
  feed      the feed launch alone

Both steppers train their own copy of the model through ``train._SampleStepper``, the code ``train()`` runs.  A window is ``passes``
passes over all batches closed by ONE device synchronise (the loop synchronises once per epoch); windows of the three modes alternate
inside every round, and the median / min / max over rounds are printed per batch.  32 distinct batches: the topology cache
(16 entries, keyed by tensor identity) never hits, as with a loader that builds new tensors for every batch.

    python tools/latency_ragged_batch.py [rounds=9] [batches=32] [passes=4]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphnet_classifier_amd import synthetic  # noqa: E402
from graphnet_classifier_amd.GNN import CombinedModel, GraphNet  # noqa: E402
from graphnet_classifier_amd.train import FlatParameters, FusedAdam, _SampleStepper  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 32
PASSES = int(sys.argv[3]) if len(sys.argv) > 3 else 4  # passes over the batches per timed window
G = 8
DEV = torch.device("cuda:0")


def stepper(capture: bool):
    torch.manual_seed(0)
    model = CombinedModel(GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=156, classes=2)
    model.ragged_readout = True
    model.train()
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    return _SampleStepper(model, FusedAdam(FlatParameters(model), lr=1e-3), torch.nn.CrossEntropyLoss(), loss_sum, DEV, capture)


def main():
    batches = [synthetic.superpixel_like_graphs(G, seed=3000 + k).to(DEV) for k in range(BATCHES)]
    labels = [torch.tensor([(k + g) % 2 for g in range(G)]) for k in range(BATCHES)]
    nodes, edges = [b.num_nodes for b in batches], [b.num_edges for b in batches]
    print(f"{BATCHES} batches of {G} graphs: {min(nodes)}-{max(nodes)} nodes, {min(edges)}-{max(edges)} edges per batch", flush=True)
    eager, captured = stepper(False), stepper(True)

    def run(step):
        for b, lab in zip(batches, labels):
            step(b, lab)

    for _ in range(2):  # warm-up of every shape the windows use; the second batch of the first pass makes the capture
        run(eager)
        run(captured)
    torch.cuda.synchronize()
    cap = captured.ragged.current
    assert cap is not None and captured.ragged.captures == 1 and all(cap.matches(b) for b in batches), "the stream must replay one capture"
    print(f"captured at node_capacity {cap.node_capacity}, edge_capacity {cap.edge_capacity} ({cap.feed.rows} rows)", flush=True)

    def feed_only(b, lab):
        cap.feed(b, lab)

    modes = {"eager": eager, "captured": captured, "feed": feed_only}
    times = {name: [] for name in modes}
    for _ in range(ROUNDS):
        for name, step in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(PASSES):
                run(step)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / (PASSES * BATCHES))
    captured.check()
    for name, ts in times.items():
        ms = 1e3 * np.asarray(ts)
        print(f"{name:9s} per batch: median {np.median(ms):8.4f} ms   min {ms.min():8.4f}   max {ms.max():8.4f}   ({ROUNDS} windows of {PASSES} x {BATCHES} batches)")
    ratio = np.median(times["eager"]) / np.median(times["captured"])
    print(f"eager / captured = {ratio:.2f}x")
    le, lc = float(eager.loss_sum.item()), float(captured.loss_sum.item())
    print(f"loss accumulated over the same steps: eager {le:.6f} captured {lc:.6f} (relative difference {abs(le - lc) / abs(le):.2e})")


if __name__ == "__main__":
    main()
