#!/usr/bin/env python3
"""What the training controls of DESIGN K22 cost inside the captured single-graph training step, on one device.

Workload: the reference's own regime - one graph per optimizer step - at the ~1000-node size the README quotes: a 32 x 32 pixel
graph (N = 1024, E = 1984) through the default model (D = 128, 3 GN blocks, main.py:72), the whole step (forward + CE + backward +
gradient pack + optimizer) replayed from ONE hipGraph (``train.CapturedTrainStep``), inputs resident on the device.

Variants, one model, optimizer and capture each, same seed:
  plain_adam          ``FusedAdam(lr=1e-3)``: the default path, two launches (tick + element)
  adamw               decoupled weight decay: the controlled path, two launches (control tick + element)
  adamw_clip          + ``max_grad_norm``: three launches (the sum-of-squares pass in front)
  adamw_clip_cosine   + warm-up and cosine decay: the same three launches, the schedule evaluated in the tick
  sgd                 ``FusedSGD(momentum=0.9)``: two launches, one state buffer less to stream

Timing (measuring-on-mi355x, section 5): every capture warmed up, then ``rounds`` rounds in which windows of ``iters`` replays of
the variants alternate in this one process; a window is ONE pair of HIP events with a synchronise behind it and lasts about a
second at the default ``iters``.  Median / min / max over the rounds, ms per step, and each variant's median over plain_adam's.
Results go to ``profiles/optimizer_controls.json``.

    python tools/bench_optimizer_controls.py [rounds=5] [iters=2000] [out=profiles/optimizer_controls.json] [variants=all]

``variants`` is a comma-separated subset (``plain_adam`` alone also runs on a tree from before K22: the check that the default path
did not move)."""
import datetime
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.environ.get("GNC_BENCH_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # another tree's package
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import native  # noqa: E402
from graphnet_classifier_amd import train as T  # noqa: E402
from graphnet_classifier_amd.GNN import CombinedModel, GraphNet  # noqa: E402
from graphnet_classifier_amd.image_to_graph import create_grid_edges_optimized  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "optimizer_controls.json")
ONLY = sys.argv[4].split(",") if len(sys.argv) > 4 and sys.argv[4] != "all" else None
DEV = torch.device("cuda:0")
SIDE = 32
COSINE = dict(kind="cosine", warmup_steps=1000, total_steps=10 ** 9, min_lr=1e-5)  # never reaches its end inside a run

VARIANTS = {
    "plain_adam": lambda fp: T.FusedAdam(fp, lr=1e-3),
    "adamw": lambda fp: T.FusedAdam(fp, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True),
    "adamw_clip": lambda fp: T.FusedAdam(fp, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0),
    "adamw_clip_cosine": lambda fp: T.FusedAdam(fp, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1.0,
                                                lr_schedule=COSINE),
    "sgd": lambda fp: T.FusedSGD(fp, 1e-3, momentum=0.9),
}
OPTIMIZER_LAUNCHES = {"plain_adam": 2, "adamw": 2, "adamw_clip": 3, "adamw_clip_cosine": 3, "sgd": 2}


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per step


def sample():
    rr, cc = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(SIDE * SIDE, 3, generator=gen) * 255
    pos = torch.from_numpy(np.stack([rr.ravel(), cc.ravel()], 1).astype(np.float32))
    return x, pos, create_grid_edges_optimized(SIDE, SIDE).cpu()


def capture(make, graph):
    torch.manual_seed(0)
    model = CombinedModel(GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=SIDE * SIDE, classes=2)
    model.train()
    opt = make(T.FlatParameters(model))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    step = T.CapturedTrainStep(model, opt, torch.nn.CrossEntropyLoss(), graph, torch.tensor(1), loss_sum)
    return step, opt, loss_sum


def main():
    assert torch.cuda.is_available(), "bench_optimizer_controls needs a GPU: there is no CPU timing of a GPU step"
    native.load_library()
    props = torch.cuda.get_device_properties(0)
    graph = sample()
    names = [n for n in VARIANTS if ONLY is None or n in ONLY]
    steps = {name: capture(VARIANTS[name], graph) for name in names}
    for step, _, _ in steps.values():
        window(step.replay, 200)
    times = {name: [] for name in names}
    for _ in range(ROUNDS):
        for name in names:
            times[name].append(window(steps[name][0].replay, ITERS))
    results = {}
    for name in names:
        step, opt, loss_sum = steps[name]
        t = times[name]
        done = int(opt.step_count.item())
        results[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "window_s": statistics.median(t) * ITERS / 1e3,
                         "optimizer_launches": OPTIMIZER_LAUNCHES[name], "steps_run": done,
                         "mean_loss": float(loss_sum.item()) / max(1, done), "parameters_finite": bool(torch.isfinite(opt.fp.flat).all())}
        for key in ("current_lr", "grad_norm", "skipped_steps"):  # a tree from before K22 has none of them
            if hasattr(opt, key):
                value = float(getattr(opt, key).item())
                results[name][key] = value if value == value else None  # grad_norm is NaN when no norm pass runs
    base = results.get("plain_adam")
    for name, r in results.items():
        if base is not None:
            r["over_plain_adam_us"] = (r["median_ms"] - base["median_ms"]) * 1e3
        print(f"{name:18s} {r['median_ms'] * 1e3:8.1f} us per step (min {r['min_ms'] * 1e3:8.1f}, max {r['max_ms'] * 1e3:8.1f}; window "
              f"{r['window_s']:.2f} s)" + (f"  {r['over_plain_adam_us']:+6.1f} us over plain_adam" if base is not None else ""), flush=True)
    doc = {"tool": "tools/bench_optimizer_controls.py", "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""),
           "compute_units": props.multi_processor_count, "date": datetime.date.today().isoformat(), "rounds": ROUNDS, "iters": ITERS,
           "workload": f"captured training step, {SIDE} x {SIDE} pixel graph (N = {SIDE * SIDE}, E = {graph[2].size(1)}), default model "
                       f"(D = 128, 3 blocks), {steps[names[0]][1].fp.numel} flat parameters",
           "timing": "HIP events around windows of `iters` graph replays, the variants' windows alternating in one process; ms per step",
           "variants": results}
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
