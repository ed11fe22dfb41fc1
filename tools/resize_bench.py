#!/usr/bin/env python3
"""Throughput of the device resize (csrc/resize.hip) and of the image-folder loader (graphnet_classifier_amd/dataset.py).

    python tools/resize_bench.py [--batches 1,64,256] [--iters 5] [--images 256] [--workers 16]

Prints one JSON line per measurement:
  resize       device resize of a dense uint8 batch already in HBM (500x375 -> 128 and 2000x1500 -> 128): hipEvent time,
               median of --iters calls after a warm-up; GB/s counts the input bytes read once plus the output written.
  host_resize  HOST ONLY: PIL Image.resize of one image on one core (median of --iters), the step the device resize
               replaces in the single-image builders.
  loader       one epoch over a generated folder of --images JPEGs (500x375) in 2 classes: GraphImageFolder.loader()
               with --workers decode threads, against the per-image loop the reference runs (PIL open, convert, resize,
               one single-image builder call, in order, one thread); samples/s, wall clock, GPU synchronised at the end.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graphnet_classifier_amd import dataset as D  # noqa: E402
from graphnet_classifier_amd import image_to_graph as I2G  # noqa: E402

CASES = [((375, 500), 128), ((1500, 2000), 128)]


def photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 120 * np.sin(xx / rng.uniform(5, 60) + c) * np.cos(yy / rng.uniform(5, 60)) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def bench_resize(batches, iters):
    from PIL import Image
    for (h, w), R in CASES:
        base = [photo(h, w, k) for k in range(4)]
        for B in batches:
            src = torch.from_numpy(np.stack([base[k % 4] for k in range(B)])).cuda()
            ms = timed(lambda: I2G.resize(src, (R, R)), iters)
            nbytes = B * (h * w * 3 + R * R * 3)
            print(json.dumps({"bench": "resize", "in": f"{w}x{h}", "out": R, "B": B, "ms": round(ms, 4),
                              "images_per_s": round(B / ms * 1e3, 1), "GB_per_s": round(nbytes / ms / 1e6, 1)}),
                  flush=True)
            del src
        pil = Image.fromarray(base[0])
        host = []
        for _ in range(iters + 1):
            t0 = time.perf_counter()
            pil.resize((R, R))
            host.append(time.perf_counter() - t0)
        ms = float(np.median(host[1:])) * 1e3
        print(json.dumps({"bench": "host_resize", "host_only": True, "in": f"{w}x{h}", "out": R, "ms": round(ms, 3),
                          "images_per_s": round(1e3 / ms, 1)}), flush=True)


def bench_loader(n_images, workers):
    from PIL import Image
    with tempfile.TemporaryDirectory() as root:
        for k in range(n_images):
            d = os.path.join(root, f"class{k % 2}")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(photo(375, 500, 100 + k)).save(os.path.join(d, f"img{k:04d}.jpg"), quality=90)
        for method in ("pixel", "superpixel"):
            ds = D.GraphImageFolder(root, resize_value=128, method=method)
            single = {"pixel": I2G.image_to_graph_pixel_optimized, "superpixel": I2G.image_to_graph_superpixel}[method]
            results = {}
            for name in ("reference_loop", "loader"):
                for _ in range(2):  # the first pass builds caches (grid edges, code objects)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    count = 0
                    if name == "loader":
                        for g, _ in ds.loader(workers=workers):
                            count += 1
                    else:
                        for path, label in ds.samples:
                            g = single(Image.open(path).convert("RGB"))
                            count += 1
                    torch.cuda.synchronize()
                    results[name] = count / (time.perf_counter() - t0)  # the second pass is kept
            print(json.dumps({"bench": "loader", "method": method, "images": n_images, "in": "500x375 jpeg", "R": 128,
                              "workers": workers, "loader_samples_per_s": round(results["loader"], 1),
                              "reference_loop_samples_per_s": round(results["reference_loop"], 1),
                              "speedup": round(results["loader"] / results["reference_loop"], 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    bench_resize([int(v) for v in args.batches.split(",")], args.iters)
    bench_loader(args.images, args.workers)


if __name__ == "__main__":
    main()
