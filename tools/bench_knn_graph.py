#!/usr/bin/env python3
"""Measures the k-nearest-neighbour graph build (DESIGN K24) on the GPU and writes profiles/knn_graph.json.

Baseline: the same edge list from ``torch`` ops in the same process - ``cdist(...)**2`` + ``topk`` per graph, concatenated (ties
broken however ``topk`` likes: only the time is compared).  Device events around windows of calls, a warm-up of every shape,
medians over repeats, the two sides alternating inside every repeat.

    python tools/bench_knn_graph.py [--out profiles/knn_graph.json] [--repeats 5] [--skip-train]

The default path (``edges=None``) against another tree, e.g. the parent commit with its own library - fresh processes, alternating:

    [GNC_BENCH_ROOT=<tree>] python tools/bench_knn_graph.py --default-loader        # one JSON line: the loader chunk, 15 calls
    (cd <tree> && python bench.py --gpus 1 --steps 20 --warmup 5)                  # the flagship benchmark of that tree
    python tools/bench_knn_graph.py --record-default <log of those lines> --out profiles/knn_graph.json

A developer build of the kernel (``make -C graphnet_classifier_amd/csrc variant UNIT=knn_graph V=grouped
EXTRA=-DGNC_KNN_GROUPED_LOADS``) beside the shipped one - its own process, the same session, added to the same file:

    GNC_LIB_PATH=build/libgnc_grouped.so python tools/bench_knn_graph.py --kernel-variant grouped_loads --out profiles/knn_graph.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("GNC_BENCH_ROOT", ROOT))  # the tree whose package is measured (--default-loader: maybe another)

from graphnet_classifier_amd import functional as F  # noqa: E402
from graphnet_classifier_amd import image_to_graph as I2G  # noqa: E402
from graphnet_classifier_amd import native, synthetic  # noqa: E402


def window_ms(fn, iters):
    """Mean milliseconds of ``fn`` over one window of ``iters`` calls (device events)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(sides, iters, repeats):
    """{name: median ms} of several callables, alternating inside every repeat; ``iters``: {name: calls per window}."""
    for name, fn in sides.items():  # warm-up of every shape
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            samples[name].append(window_ms(fn, iters[name]))
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_per_window": iters[name],
                   "windows": repeats} for name, v in samples.items()}


def torch_knn(feat, ptr, k):
    """cdist + topk per graph, concatenated: [2, k N] with the kernel's layout."""
    out = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        f = feat[a:b]
        d = torch.cdist(f, f).square_()
        d.fill_diagonal_(float("inf"))
        idx = torch.topk(d, k, dim=1, largest=False, sorted=True).indices + a
        recv = torch.arange(a, b, device=feat.device).repeat_interleave(k)
        out.append(torch.stack([idx.reshape(-1), recv]))
    return torch.cat(out, dim=1)


def graph_shapes(rng, num_graphs, lo, hi):
    sizes = rng.integers(lo, hi + 1, num_graphs)
    return [0] + np.cumsum(sizes).tolist()


def bench_kernel(repeats):
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    results = {}
    k = 8

    # a chunk of 64 superpixel graphs (80 .. 120 nodes), both entries
    ptr = graph_shapes(rng, 64, 80, 120)
    N = ptr[-1]
    feat = torch.from_numpy(rng.random((N, 5), dtype=np.float32)).to(dev)
    gp = torch.tensor(ptr, dtype=torch.int64, device=dev)
    cap = 160
    padded = torch.zeros(64, cap, 5, device=dev)
    counts = torch.zeros(64, 4, dtype=torch.int32, device=dev)
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        padded[g, :b - a] = feat[a:b]
        counts[g, 0] = b - a
    results["chunk_64_superpixel_graphs"] = {
        "nodes": N, "k": k, "dim": 5, "node_capacity": cap,
        **alternate({"hip_graph_ptr": lambda: F.knn_graph(feat, k, graph_ptr=gp),
                     "hip_padded": lambda: native.knn_graph_padded(padded, counts, k),
                     "torch_cdist_topk": lambda: torch_knn(feat, ptr, k)},
                    {"hip_graph_ptr": 200, "hip_padded": 200, "torch_cdist_topk": 5}, repeats)}

    # one 16,384-node pixel graph
    N = 16384
    feat1 = torch.from_numpy(rng.random((N, 5), dtype=np.float32)).to(dev)
    gp1 = torch.tensor([0, N], dtype=torch.int64, device=dev)
    results["one_16384_node_graph"] = {
        "nodes": N, "k": k, "dim": 5,
        **alternate({"hip_graph_ptr": lambda: F.knn_graph(feat1, k, graph_ptr=gp1),
                     "torch_cdist_topk": lambda: torch_knn(feat1, [0, N], k)},
                    {"hip_graph_ptr": 20, "torch_cdist_topk": 5}, repeats)}

    # what a pixel chunk of the loader at its default resize_value = 128 is: 64 graphs of 16,384 nodes
    N = 64 * 16384
    ptr3 = [16384 * g for g in range(65)]
    feat3 = torch.from_numpy(rng.random((N, 5), dtype=np.float32)).to(dev)
    gp3 = torch.tensor(ptr3, dtype=torch.int64, device=dev)
    results["pixel_chunk_64_graphs_of_16384_nodes"] = {
        "nodes": N, "k": k, "dim": 5,
        **alternate({"hip_graph_ptr": lambda: F.knn_graph(feat3, k, graph_ptr=gp3),
                     "torch_cdist_topk": lambda: torch_knn(feat3, ptr3, k)},
                    {"hip_graph_ptr": 2, "torch_cdist_topk": 1}, 3)}

    # 10,000 graphs of about 150 nodes
    ptr2 = graph_shapes(rng, 10000, 120, 180)
    N = ptr2[-1]
    feat2 = torch.from_numpy(rng.random((N, 5), dtype=np.float32)).to(dev)
    gp2 = torch.tensor(ptr2, dtype=torch.int64, device=dev)
    results["10000_graphs_of_150_nodes"] = {
        "nodes": N, "k": k, "dim": 5,
        **alternate({"hip_graph_ptr": lambda: F.knn_graph(feat2, k, graph_ptr=gp2),
                     "torch_cdist_topk": lambda: torch_knn(feat2, ptr2, k)},
                    {"hip_graph_ptr": 5, "torch_cdist_topk": 1}, max(3, repeats // 2 + 1))}
    return results


def photos(count, side, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    out = []
    for _ in range(count):
        chans = [127 + 120 * np.sin(xx / rng.uniform(5, 40) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(5, 40)) for _ in range(3)]
        out.append(np.clip(np.stack(chans, -1) + rng.normal(0, 6, (side, side, 3)), 0, 255).astype(np.uint8))
    return out


def host_ms(fn, repeats):
    """Median host milliseconds of calls that end in a device synchronise."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return out


def default_loader():
    """One process's figure of the default path: the edges=None build of the chunk ``bench_loader`` uses, 15 synchronised calls."""
    images = photos(64, 128, 5)
    v = host_ms(lambda: I2G.graphs_from_images(images, "superpixel", resize_value=128, n_segments=100), 15)
    return {"tree": os.path.dirname(os.path.dirname(os.path.abspath(I2G.__file__))), "loader_chunk_ms_median": statistics.median(v),
            "min_ms": min(v), "max_ms": max(v), "calls": len(v)}


def record_default(log, out):
    """Adds the alternating default-path runs of ``log`` to ``out``: lines ``== <tree> run <i>`` followed by bench.py's result line
    and a --default-loader line."""
    runs, tree = {}, None
    for line in open(log):
        line = line.strip()
        if line.startswith("== "):
            tree = line.split()[1]
            runs.setdefault(tree, {"bench_py_ms_per_step": [], "loader_chunk_edges_none_ms": []})
        elif line.startswith("{") and tree:
            rec = json.loads(line)
            if "ms_per_step" in rec:
                runs[tree]["bench_py_ms_per_step"].append(rec["ms_per_step"])
            elif "loader_chunk_ms_median" in rec:
                runs[tree]["loader_chunk_edges_none_ms"].append(rec["loader_chunk_ms_median"])
    result = json.load(open(out))
    result["default_path"] = {"method": "fresh processes alternating the trees in one session; bench.py --gpus 1 --steps 20 --warmup 5 "
                              "and tools/bench_knn_graph.py --default-loader (median of 15 synchronised calls per process)", **runs}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["default_path"]))


def bench_loader(repeats):
    """The loader's graph build of one chunk of 64 decoded 128 x 128 images (superpixel, n_segments = 100)."""
    images = photos(64, 128, 5)
    sides = {"edges_none": lambda: I2G.graphs_from_images(images, "superpixel", resize_value=128, n_segments=100),
             "edges_knn": lambda: I2G.graphs_from_images(images, "superpixel", resize_value=128, n_segments=100, edges="knn", knn_k=8)}
    samples = {name: [] for name in sides}
    for name, fn in sides.items():
        fn()
    for _ in range(repeats):
        for name, fn in sides.items():
            samples[name] += host_ms(fn, 2)
    graphs = sides["edges_none"]()
    return {"images": 64, "resize_value": 128, "n_segments": 100, "knn_k": 8,
            "mean_nodes": float(np.mean([g[0].size(0) for g in graphs])),
            "mean_rag_edges": float(np.mean([g[2].size(1) for g in graphs])),
            **{name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v)} for name, v in samples.items()}}


def bench_train(repeats, out_dir):
    """The captured per-sample training step on ONE superpixel graph: its region-adjacency edges against kNN at k = 8.  A step's
    time is the difference of two ``train()`` runs of 4 and 1 epochs over 300 copies of the sample, over the 900 steps between."""
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import train
    image = photos(1, 128, 9)
    x, pos, rag = I2G.graphs_from_images(image, "superpixel", resize_value=128, n_segments=100)[0]
    _, _, knn = I2G.graphs_from_images(image, "superpixel", resize_value=128, n_segments=100, edges="knn", knn_k=8)[0]
    label = torch.tensor(1)
    samples = {"rag": (x, pos, rag), "knn_k8": (x, pos, knn)}

    def run(sample, epochs, tag):
        torch.manual_seed(0)
        model = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(128, 3)), num_nodes=x.size(0), classes=2).cuda()
        data = [(sample, label)] * 300
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = train(model, data, epochs, patience=100, output_path=os.path.join(out_dir, tag))
        torch.cuda.synchronize()
        assert r["captured"], "the fixed-topology capture did not take the sample"
        return time.perf_counter() - t

    steps = {name: [] for name in samples}
    for name, s in samples.items():
        run(s, 1, "warm_" + name)
    repeats = max(3, repeats)
    for rep in range(repeats):
        for name, s in samples.items():
            long, short = run(s, 4, f"{name}_{rep}_4"), run(s, 1, f"{name}_{rep}_1")
            steps[name].append(1e3 * (long - short) / 900.0)
    return {"nodes": int(x.size(0)), "rag_edges": int(rag.size(1)), "knn_edges": int(knn.size(1)), "width": 128, "n_blocks": 3,
            **{name: {"median_step_ms": statistics.median(v), "min_step_ms": min(v), "max_step_ms": max(v), "repeats": len(v)}
               for name, v in steps.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_graph.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--default-loader", action="store_true", help="print this process's edges=None loader figure and exit")
    ap.add_argument("--record-default", metavar="LOG", help="add the default-path runs of LOG to --out and exit")
    ap.add_argument("--kernel-variant", metavar="NAME", help="measure the kernel shapes with the library of GNC_LIB_PATH and add them "
                    "to --out as kernel_variant_NAME")
    ap.add_argument("--scratch", default=None, help="directory for the training runs' logs and checkpoints (a temporary one by default)")
    a = ap.parse_args()
    if a.record_default:
        return record_default(a.record_default, a.out)
    if not torch.cuda.is_available():
        sys.exit("bench_knn_graph: needs a GPU (nothing here is measured on a CPU)")
    native.load_library()
    if a.default_loader:
        print(json.dumps(default_loader()))
        return
    if a.kernel_variant:
        result = json.load(open(a.out))
        result["kernel_variant_" + a.kernel_variant] = {"library": os.environ.get("GNC_LIB_PATH", native.LIB_PATH), **bench_kernel(a.repeats)}
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result["kernel_variant_" + a.kernel_variant]))
        return
    import tempfile
    result = {"device": torch.cuda.get_device_name(0), "method": "device events per window of calls (kernel) / host clock around a "
              "synchronised call (loader, train); medians, sides alternating inside every repeat",
              "kernel": bench_kernel(a.repeats)}
    print(json.dumps(result["kernel"]), flush=True)
    result["loader_chunk"] = bench_loader(a.repeats)
    print(json.dumps(result["loader_chunk"]), flush=True)
    if not a.skip_train:
        with tempfile.TemporaryDirectory(dir=a.scratch) as tmp:
            result["captured_train_step"] = bench_train(a.repeats // 2, tmp)
        print(json.dumps(result["captured_train_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
