#!/usr/bin/env python3
"""Per-image time of the device SLIC (csrc/superpixel.hip) and of image -> superpixel graph.

    python tools/superpixel_bench.py [--batches 1,16,64,256] [--sizes 64,128,256] [--iters 5]

Images are the fixture photos of tests/golden/g10_superpixel.npz (resized with PIL to each size), repeated to fill
the batch.  Times are hipEvent intervals after a warm-up call, median of --iters calls, divided by the batch size.
`graph` is slic over the batch followed by one gnc_rag_build per image (its node and edge counts are data dependent,
so each image costs one host synchronisation there).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graphnet_classifier_amd import image_to_graph as I2G  # noqa: E402


def photos(size):
    from PIL import Image
    with np.load(os.path.join(ROOT, "tests", "golden", "g10_superpixel.npz")) as z:
        imgs = [z[k] for k in z.files if k.startswith("img_") and z[k].shape == (128, 128, 3)]
    return [np.array(Image.fromarray(im).resize((size, size))) for im in imgs]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    for R in (int(v) for v in args.sizes.split(",")):
        base = photos(R)
        for B in (int(v) for v in args.batches.split(",")):
            batch = torch.from_numpy(np.stack([base[i % len(base)] for i in range(B)])).cuda()

            def graphs():
                labels = I2G.slic(batch)
                for i in range(B):
                    I2G._superpixel_graph_from_device_labels(batch[i], labels[i])

            t_slic = timed(lambda: I2G.slic(batch), args.iters)
            t_graph = timed(graphs, args.iters)
            print(json.dumps({"R": R, "B": B, "slic_ms_per_image": round(t_slic / B, 4),
                              "graph_ms_per_image": round(t_graph / B, 4), "slic_ms_batch": round(t_slic, 3)}),
                  flush=True)


if __name__ == "__main__":
    main()
