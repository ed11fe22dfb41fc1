#!/usr/bin/env python3
"""Measures the train-time augmentation (DESIGN K25) on the GPU and writes profiles/augment.json.

A loader chunk is ``image_to_graph.graphs_from_images`` of 64 decoded photographs of mixed sizes (375 x 500 and the like) at
``resize_value=128``: plain, and with the parameters an ``Augmentation`` (crop, flip, three jitters) samples for them, for
``method="pixel"`` and ``"superpixel"``.  Both sides run in the same process, alternating inside every repeat; a call is timed on
the host clock around a device synchronise, the sampling on the host included.  The two new launches are also timed alone
(device events around windows of calls) beside the plain ``resize`` of the same images.

    python tools/bench_augment.py [--out profiles/augment.json] [--repeats 7]
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
sys.path.insert(0, ROOT)

from graphnet_classifier_amd import image_to_graph as I2G  # noqa: E402
from graphnet_classifier_amd import native  # noqa: E402
from graphnet_classifier_amd.augment import Augmentation  # noqa: E402

SHAPES = [(375, 500), (500, 375), (333, 500), (480, 640)]
CHUNK, RES = 64, 128


def photos(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        h, w = SHAPES[k % len(SHAPES)]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        chans = [127 + 120 * np.sin(xx / rng.uniform(10, 90) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(10, 90)) for _ in range(3)]
        out.append(np.clip(np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def window_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def summary(v, **extra):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v), **extra}


def bench_chunks(images, aug, repeats):
    sizes = [im.shape[:2] for im in images]
    epoch = [0]

    def augmented(method):
        epoch[0] += 1  # other crops every call, as in training
        params = aug.sample(sizes, epoch[0], range(len(images)))
        return I2G.graphs_from_images(images, method, resize_value=RES, n_segments=100, augmentation=params)

    out = {}
    for method in ("pixel", "superpixel"):
        sides = {"plain": lambda: I2G.graphs_from_images(images, method, resize_value=RES, n_segments=100),
                 "augmented": lambda: augmented(method)}
        samples = {name: [] for name in sides}
        for fn in sides.values():
            fn()
            fn()
        for _ in range(repeats):
            for name, fn in sides.items():
                samples[name] += [host_ms(fn), host_ms(fn)]
        out[method] = {name: summary(v) for name, v in samples.items()}
        out[method]["augmented_minus_plain_ms"] = out[method]["augmented"]["median_ms"] - out[method]["plain"]["median_ms"]
    t = []
    for e in range(20):
        t0 = time.perf_counter()
        aug.sample(sizes, 1000 + e, range(len(images)))
        t.append(1e3 * (time.perf_counter() - t0))
    out["host_sampling_of_the_chunk"] = summary(t)
    return out


def bench_launches(images, aug, repeats):
    """The launches alone, inputs already on the device: resize and crop_resize of the packed mixed-size chunk, color_jitter on the
    resized batch."""
    dev = [torch.from_numpy(im).cuda() for im in images]
    params = aug.sample([im.shape[:2] for im in images], 1, range(len(images)))
    batch = I2G.resize(dev, (RES, RES))
    sides = {"resize": lambda: I2G.resize(dev, (RES, RES)),
             "crop_resize": lambda: I2G.crop_resize(dev, params.boxes, (RES, RES), "bicubic", params.flips),
             "color_jitter_3_operations": lambda: I2G.color_jitter(batch, params.brightness, params.contrast, params.saturation, params.order),
             "color_jitter_brightness_alone": lambda: I2G.color_jitter(batch, brightness=params.brightness),
             "copy_of_the_batch": lambda: batch.clone()}
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            samples[name].append(window_ms(fn, 50))
    return {"note": "each call includes the wrapper's packing of the device images / its copy of the batch; 50 calls per window",
            **{name: summary(v, ms_per_image=statistics.median(v) / len(images)) for name, v in samples.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment: needs a GPU (nothing here is measured on a CPU)")
    native.load_library()
    images = photos(CHUNK, 5)
    aug = Augmentation(brightness=0.4, contrast=0.4, saturation=0.4, seed=1)
    result = {"device": torch.cuda.get_device_name(0), "images": CHUNK, "image_sizes": SHAPES, "resize_value": RES,
              "augmentation": "scale (0.08, 1), ratio (3/4, 4/3), hflip 0.5, brightness / contrast / saturation 0.4",
              "method": "host clock around a synchronised graphs_from_images call of host images (chunk) / device events per window of "
                        "calls (launches); medians, sides alternating inside every repeat, same process"}
    result["loader_chunk"] = bench_chunks(images, aug, a.repeats)
    print(json.dumps(result["loader_chunk"]), flush=True)
    result["launches"] = bench_launches(images, aug, a.repeats)
    print(json.dumps(result["launches"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
