#!/usr/bin/env python3
"""What the device loss head of DESIGN K23 costs and saves, on one device.

Parts (``parts`` is a comma-separated subset; ``step_default`` alone also runs on a tree from before K23 - ``GNC_BENCH_ROOT`` names
the tree whose package is measured - which is the check that the default path did not move):

  step       the captured single-graph training step of tools/bench_optimizer_controls.py - a 32 x 32 pixel graph (N = 1024,
             E = 1984) through the default model (D = 128, 3 GN blocks), forward + loss + backward + gradient pack + Adam replayed
             from ONE hipGraph - with three criteria, one model, optimizer and capture each, same seed:
               default      ``nn.CrossEntropyLoss()`` on PyTorch's ops (``train(loss=None)``)
               ce           ``ClassificationLoss("ce")`` bound to the loss accumulator (``train(loss="ce")``)
               ce_metrics   the same with the confusion counts (``metrics=True``)
             Windows of ``iters`` replays of the three alternate in this one process for ``rounds`` rounds.
  evaluate   ``train.evaluate`` over 50 mini-batches of 8 graphs (144 nodes each), with and without ``criterion=``: host clock around
             the call (it ends in its one host read), per batch.
  head       the head alone at G = 10,000, C = 2 (three launches: rows, tick, gradient) beside ``F.cross_entropy`` forward + backward
             in torch ops, windows of ``iters`` calls.
  launches   device kernels of ONE eager training step under each criterion (torch.profiler's device events) and the library's own
             share of them (``KernelTimers.num_launches``: one entry per wrapper call).

Timing (measuring-on-mi355x, section 5): everything warmed up; a window is ONE pair of HIP events with a synchronise behind it.
Median / min / max over the rounds.  Results go to ``profiles/loss_head.json``.

    python tools/bench_loss_head.py [rounds=5] [iters=2000] [out=profiles/loss_head.json] [parts=all]
"""
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.environ.get("GNC_BENCH_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # another tree's package
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import native, synthetic  # noqa: E402
from graphnet_classifier_amd import train as T  # noqa: E402
from graphnet_classifier_amd.GNN import CombinedModel, GraphNet  # noqa: E402
from graphnet_classifier_amd.image_to_graph import create_grid_edges_optimized  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "loss_head.json")
PARTS = sys.argv[4].split(",") if len(sys.argv) > 4 and sys.argv[4] != "all" else ["step", "evaluate", "head", "launches"]
DEV = torch.device("cuda:0")
SIDE = 32
HEAD_ROWS = 10_000


def criterion(name):
    if name == "default":
        return torch.nn.CrossEntropyLoss()
    from graphnet_classifier_amd.loss import ClassificationLoss
    return ClassificationLoss("ce", track_metrics=name == "ce_metrics")


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms per call


def stats(t, unit=1e3):
    return {"median_us": statistics.median(t) * unit, "min_us": min(t) * unit, "max_us": max(t) * unit}


def sample():
    rr, cc = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(SIDE * SIDE, 3, generator=gen) * 255
    pos = torch.from_numpy(np.stack([rr.ravel(), cc.ravel()], 1).astype(np.float32))
    return x, pos, create_grid_edges_optimized(SIDE, SIDE).cpu()


def model_and_optimizer():
    torch.manual_seed(0)
    model = CombinedModel(GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=SIDE * SIDE, classes=2)
    model.train()
    return model, T.FusedAdam(T.FlatParameters(model), lr=1e-3)


def part_step(names):
    graph = sample()
    steps = {}
    for name in names:
        model, opt = model_and_optimizer()
        loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
        crit = criterion(name)
        if hasattr(crit, "bind_loss_sum"):
            crit.bind_loss_sum(loss_sum)
        steps[name] = (T.CapturedTrainStep(model, opt, crit, graph, torch.tensor(1), loss_sum), opt, loss_sum, crit)
    for step, _, _, _ in steps.values():
        window(step.replay, 200)
    times = {name: [] for name in names}
    for _ in range(ROUNDS):
        for name in names:
            times[name].append(window(steps[name][0].replay, ITERS))
    out = {}
    for name in names:
        step, opt, loss_sum, crit = steps[name]
        done = int(opt.step_count.item())
        out[name] = dict(stats(times[name]), window_s=statistics.median(times[name]) * ITERS / 1e3, steps_run=done,
                         mean_loss=float(loss_sum.item()) / max(1, done), parameters_finite=bool(torch.isfinite(opt.fp.flat).all()))
        if getattr(crit, "confusion", None) is not None:
            out[name]["samples_counted"] = int(crit.confusion.sum())
    base = out.get("default")
    for name, r in out.items():
        if base is not None:
            r["over_default_us"] = r["median_us"] - base["median_us"]
        print(f"step {name:11s} {r['median_us']:8.1f} us (min {r['min_us']:8.1f}, max {r['max_us']:8.1f}; window {r['window_s']:.2f} s)"
              + (f"  {r['over_default_us']:+6.1f} us over default" if base is not None else ""), flush=True)
    return out


def part_evaluate():
    from graphnet_classifier_amd.loss import ClassificationLoss
    torch.manual_seed(0)
    model = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(128, 3)), num_nodes=144, classes=2).eval()
    batches = [synthetic.superpixel_like_graphs(8, 100 + i, shapes=((12, 12),)) for i in range(50)]
    gen = torch.Generator().manual_seed(1)
    loader = [(b, torch.randint(0, 2, (8,), generator=gen)) for b in batches]
    crit = ClassificationLoss("ce")
    forms = {"torch_ops": lambda: T.evaluate(model, loader, capture=False),
             "criterion": lambda: T.evaluate(model, loader, capture=False, criterion=crit)}
    results, times = {}, {k: [] for k in forms}
    for fn in forms.values():
        fn()
    for _ in range(ROUNDS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            started = time.perf_counter()
            results[name] = fn()
            times[name].append((time.perf_counter() - started) / len(loader))  # seconds per batch
    out = {name: dict(stats(times[name], 1e6), loss=results[name]["loss"], accuracy=results[name]["accuracy"]) for name in forms}
    out["same_confusion"] = bool(torch.equal(results["torch_ops"]["confusion"], results["criterion"]["confusion"]))
    for name in forms:
        print(f"evaluate {name:10s} {out[name]['median_us']:8.1f} us per batch of 8 (min {out[name]['min_us']:8.1f}, max "
              f"{out[name]['max_us']:8.1f})", flush=True)
    return out


def part_head():
    gen = torch.Generator().manual_seed(2)
    z = (torch.randn(HEAD_ROWS, 2, generator=gen) * 3).to(DEV)
    y = torch.randint(0, 2, (HEAD_ROWS,), generator=gen).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    work = torch.zeros(native.CLASS_LOSS_WORKSPACE_DOUBLES, dtype=torch.float64, device=DEV)
    leaf = z.clone().requires_grad_(True)

    def torch_ops():
        leaf.grad = None
        torch.nn.functional.cross_entropy(leaf, y).backward()

    forms = {"class_loss": lambda: native.class_loss(z, y, status=status, workspace=work), "torch_ops": torch_ops}
    times = {k: [] for k in forms}
    for fn in forms.values():
        window(fn, 200)
    for _ in range(ROUNDS):
        for name, fn in forms.items():
            times[name].append(window(fn, ITERS))
    loss, dz = forms["class_loss"]()
    torch_ops()
    out = {name: stats(times[name]) for name in forms}
    out["class_loss"]["kernel_launches"] = native.class_loss_launches(HEAD_ROWS)
    out["max_abs_gradient_difference"] = float((dz - leaf.grad).abs().max())
    out["note"] = "per call from a host loop, enqueue included"
    for name in forms:
        print(f"head G={HEAD_ROWS} C=2 {name:10s} {out[name]['median_us']:8.1f} us per call (min {out[name]['min_us']:8.1f}, max "
              f"{out[name]['max_us']:8.1f})", flush=True)
    return out


def part_launches():
    from torch.profiler import ProfilerActivity, profile
    graph = sample()
    out = {}
    for name in ("default", "ce", "ce_metrics"):
        model, opt = model_and_optimizer()
        loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
        crit = criterion(name)
        if hasattr(crit, "bind_loss_sum"):
            crit.bind_loss_sum(loss_sum)
        stepper = T._SampleStepper(model, opt, crit, loss_sum, DEV, capture=False)
        for _ in range(3):
            stepper(graph, torch.tensor(1))
        timers = native.KernelTimers()
        native.set_kernel_timers(timers)
        stepper(graph, torch.tensor(1))
        native.set_kernel_timers(None)
        entry = {"library_launches": timers.num_launches(), "class_loss_launches": len(timers.events.get("class_loss", []))}
        try:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                stepper(graph, torch.tensor(1))
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower()]
            entry["device_kernels"] = len(kernels)
        except Exception as exc:  # the profiler is a convenience here: say so, keep the library's own count
            entry["device_kernels"] = None
            entry["device_kernels_error"] = f"{type(exc).__name__}: {exc}"
        out[name] = entry
        print(f"launches {name:11s} {entry}", flush=True)
    return out


def main():
    assert torch.cuda.is_available(), "bench_loss_head needs a GPU: there is no CPU timing of a GPU step"
    native.load_library()
    props = torch.cuda.get_device_properties(0)
    doc = {"tool": "tools/bench_loss_head.py", "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", ""),
           "compute_units": props.multi_processor_count, "date": datetime.date.today().isoformat(), "rounds": ROUNDS, "iters": ITERS,
           "workload": f"captured training step, {SIDE} x {SIDE} pixel graph (N = {SIDE * SIDE}), default model (D = 128, 3 blocks)",
           "timing": "HIP events around windows of `iters` calls, the variants' windows alternating in one process; us per call"}
    for part in PARTS:
        if part == "step" or part.startswith("step_"):
            names = ["default", "ce", "ce_metrics"] if part == "step" else [part[len("step_"):]]
            doc["step"] = part_step(names)
        elif part == "evaluate":
            doc["evaluate"] = part_evaluate()
        elif part == "head":
            doc["head"] = part_head()
        elif part == "launches":
            doc["launches"] = part_launches()
        else:
            raise SystemExit(f"unknown part {part!r}")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
