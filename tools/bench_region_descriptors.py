#!/usr/bin/env python3
"""Measures the region descriptors (DESIGN K26) on the GPU and writes profiles/region_descriptors.json.

  launches     the descriptor launch alone beside the region-graph launch alone (gnc_rag_build_batched), both on the SLIC labels
               of 64 images of 128 x 128 at n_segments = 100, buffers allocated once (device events around windows of calls);
  loader chunk ``image_to_graph.graphs_from_images`` of 64 decoded 128 x 128 images, superpixel, with ``node_features=None`` against
               ``"descriptor"``: both in one process behind a warm-up, alternating inside every repeat, host clock around a
               device synchronise;
  train step   the captured per-sample training step on ONE superpixel graph with 3 and with 16 node columns: the difference of
               two ``train()`` runs of 4 and 1 epochs over 300 copies of the sample, over the 900 steps between (DESIGN K24);
  route        which forward kernel family the node encoder's launch takes at in_dim = 3 and 16, from the library's own query.

    python tools/bench_region_descriptors.py [--out profiles/region_descriptors.json] [--repeats 7] [--skip-train]

The default path against another tree (the parent commit), fresh processes alternating in one session:

    [GNC_BENCH_ROOT=<tree>] python tools/bench_region_descriptors.py --default-loader    # one JSON line: the plain chunk, 15 calls
    python tools/bench_region_descriptors.py --record-default <log of those lines, each behind a line "== <tree> run <i>">
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

from graphnet_classifier_amd import image_to_graph as I2G  # noqa: E402
from graphnet_classifier_amd import native, synthetic  # noqa: E402

CHUNK, RES, SEGMENTS = 64, 128, 100
WINDOW = 2000  # launches per timed window: about 0.1 s of device work


def photos(count, side, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    out = []
    for _ in range(count):
        chans = [127 + 120 * np.sin(xx / rng.uniform(5, 40) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(5, 40)) for _ in range(3)]
        out.append(np.clip(np.stack(chans, -1) + rng.normal(0, 6, (side, side, 3)), 0, 255).astype(np.uint8))
    return out


def window_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def summary(v, **extra):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v), **extra}


def bench_launches(repeats):
    lib = native.load_library()
    dev = torch.device("cuda")
    imgs = torch.from_numpy(np.stack(photos(CHUNK, RES, 5))).to(dev)
    labels = I2G.slic(imgs, n_segments=SEGMENTS, compactness=10, start_label=0).contiguous()
    nodes, edges = I2G.superpixel_capacities(SEGMENTS)
    B, H, W, _ = imgs.shape
    stream = torch.cuda.current_stream().cuda_stream
    x, pos = torch.empty(B, nodes, 3, device=dev), torch.empty(B, nodes, 2, device=dev)
    ei = torch.empty(B, 2, edges, dtype=torch.int64, device=dev)
    desc = torch.empty(B, nodes, I2G.REGION_DESCRIPTOR_DIM, device=dev)
    c4, c3 = torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, 3, dtype=torch.int32, device=dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    assert lib.gnc_rag_batched_workspace_bytes(B, H, W, nodes, edges) <= 256 >= lib.gnc_region_descriptors_workspace_bytes(B, H, W, nodes)

    def rag():
        native._check(lib.gnc_rag_build_batched(labels.data_ptr(), imgs.data_ptr(), B, H, W, nodes, edges, x.data_ptr(), pos.data_ptr(),
                                                ei.data_ptr(), c4.data_ptr(), ws.data_ptr(), 256, stream), "rag")

    def descriptor():
        native._check(lib.gnc_region_descriptors_rgb_u8(labels.data_ptr(), imgs.data_ptr(), B, H, W, nodes, desc.data_ptr(), c3.data_ptr(),
                                                        ws.data_ptr(), 256, stream), "descriptor")

    sides = {"rag_build_batched": rag, "region_descriptors": descriptor}
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    assert c3[:, 0].tolist() == c4[:, 0].tolist() and not c3[:, 1:].any() and torch.equal(desc[..., :3], x)
    samples = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            samples[name].append(window_ms(fn, WINDOW))
    return {"images": B, "size": [H, W], "n_segments": SEGMENTS, "node_capacity": nodes, "edge_capacity": edges,
            "mean_regions": float(c3[:, 0].float().mean()), "note": f"one launch per call, buffers allocated once; {WINDOW} calls per window",
            **{name: summary(v, ms_per_image=statistics.median(v) / B) for name, v in samples.items()}}


def bench_loader(repeats):
    images = photos(CHUNK, RES, 5)
    sides = {"node_features_none": lambda: I2G.graphs_from_images(images, "superpixel", resize_value=RES, n_segments=SEGMENTS),
             "node_features_descriptor": lambda: I2G.graphs_from_images(images, "superpixel", resize_value=RES, n_segments=SEGMENTS,
                                                                        node_features="descriptor")}
    for fn in sides.values():
        fn()
        fn()
    samples = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            samples[name] += [host_ms(fn), host_ms(fn)]
    out = {name: summary(v) for name, v in samples.items()}
    out["descriptor_minus_none_ms"] = out["node_features_descriptor"]["median_ms"] - out["node_features_none"]["median_ms"]
    out["spread_of_none_ms"] = out["node_features_none"]["max_ms"] - out["node_features_none"]["min_ms"]
    out["inside_the_spread"] = bool(abs(out["descriptor_minus_none_ms"]) <= out["spread_of_none_ms"])
    return {"images": CHUNK, "resize_value": RES, "n_segments": SEGMENTS, **out}


def default_loader():
    """One process's figure of the default path: the plain build of the chunk ``bench_loader`` uses, 15 synchronised calls."""
    images = photos(CHUNK, RES, 5)
    fn = lambda: I2G.graphs_from_images(images, "superpixel", resize_value=RES, n_segments=SEGMENTS)  # noqa: E731
    fn()
    fn()
    v = [host_ms(fn) for _ in range(15)]
    return {"tree": os.path.dirname(os.path.dirname(os.path.abspath(I2G.__file__))), "loader_chunk_ms_median": statistics.median(v),
            "min_ms": min(v), "max_ms": max(v), "calls": len(v)}


def record_default(log, out):
    runs, tree = {}, None
    for line in open(log):
        line = line.strip()
        if line.startswith("== "):
            tree = line.split()[1]
            runs.setdefault(tree, [])
        elif line.startswith("{") and tree:
            rec = json.loads(line)
            if "loader_chunk_ms_median" in rec:
                runs[tree].append({k: rec[k] for k in ("loader_chunk_ms_median", "min_ms", "max_ms")})
    result = json.load(open(out))
    result["default_path"] = {"method": "fresh processes alternating the trees in one session; --default-loader (node_features=None chunk, "
                              "median of 15 synchronised calls per process)",
                              **{t: {"median_of_process_medians_ms": statistics.median(r["loader_chunk_ms_median"] for r in v), "processes": v}
                                 for t, v in runs.items()}}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["default_path"]))


def node_encoder_route(graph3, graph16, widths=(32, 64, 128)):
    """The forward kernel family of the node encoder's launch, per input width, as the library's routing query answers."""
    from graphnet_classifier_amd.GNN import GraphNet
    out = {}
    for name, x in (("in_dim_3", graph3[0]), ("in_dim_16", graph16[0])):
        for width in widths:
            kw = synthetic.graphnet_kwargs(width, 2)
            kw["num_local_features"] = int(x.size(1))
            enc = GraphNet(**kw).node_encoder
            weights, biases, ln = enc._kernel_params()
            small = native.small_batch_kernel_serves([(x, None)], [w.detach() for w in weights], [b.detach() for b in biases], ln=ln)
            out[f"{name}_width_{width}_rows_{x.size(0)}"] = ("small-batch kernel (operands read in place)" if small else
                                                            "not the small-batch kernel (the weights-resident kernel up to width 64)")
    return out


def bench_train(repeats, out_dir):
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    from graphnet_classifier_amd.train import train
    image = photos(1, RES, 9)
    plain = I2G.graphs_from_images(image, "superpixel", resize_value=RES, n_segments=SEGMENTS)[0]
    wide = I2G.graphs_from_images(image, "superpixel", resize_value=RES, n_segments=SEGMENTS, node_features="descriptor")[0]
    label = torch.tensor(1)
    samples = {"F3": plain, "F16": wide}
    route = node_encoder_route(plain, wide)

    def run(sample, epochs, tag):
        torch.manual_seed(0)
        kw = synthetic.graphnet_kwargs(128, 3)
        kw["num_local_features"] = int(sample[0].size(1))
        model = CombinedModel(GraphNet(**kw), num_nodes=sample[0].size(0), classes=2).cuda()
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
    for rep in range(max(3, repeats)):
        for name, s in samples.items():
            long, short = run(s, 4, f"{name}_{rep}_4"), run(s, 1, f"{name}_{rep}_1")
            steps[name].append(1e3 * (long - short) / 900.0)
    return {"nodes": int(plain[0].size(0)), "edges": int(plain[2].size(1)), "width": 128, "n_blocks": 3,
            "node_encoder_route": route,
            **{name: {"median_step_ms": statistics.median(v), "min_step_ms": min(v), "max_step_ms": max(v), "repeats": len(v)}
               for name, v in steps.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_descriptors.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--default-loader", action="store_true", help="print this process's node_features=None loader figure and exit")
    ap.add_argument("--record-default", metavar="LOG", help="add the default-path runs of LOG to --out and exit")
    ap.add_argument("--scratch", default=None, help="directory for the training runs' logs and checkpoints (a temporary one by default)")
    a = ap.parse_args()
    if a.record_default:
        return record_default(a.record_default, a.out)
    if not torch.cuda.is_available():
        sys.exit("bench_region_descriptors: needs a GPU (nothing here is measured on a CPU)")
    native.load_library()
    if a.default_loader:
        print(json.dumps(default_loader()))
        return
    import tempfile
    result = {"device": torch.cuda.get_device_name(0),
              "method": "device events per window of calls (launches) / host clock around a synchronised call (loader chunk, train); "
                        "medians with min .. max, sides alternating inside every repeat, same process"}
    result["launches"] = bench_launches(a.repeats)
    print(json.dumps(result["launches"]), flush=True)
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
