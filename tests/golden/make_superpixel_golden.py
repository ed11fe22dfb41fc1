#!/usr/bin/env python3
"""Capture the SLIC superpixel fixtures (g10_superpixel*.npz) from scikit-image and the reference's own
``image_to_graph_superpixel``.

Run with an interpreter that has scikit-image 0.18.3 (the version the device SLIC of
``csrc/superpixel.hip`` follows), in the build container only (needs /root/reference):

    python3.9 tests/golden/make_superpixel_golden.py

The reference module imports torch at top level without using it; a stub module stands in for it.
Each image is resized once with PIL here and the uint8 array is stored, so the tests never resize.
Case arrays (one entry per case ``i``):

    img_<i>        uint8 [H, W, 3]
    labels_<i>     int32 [H, W]: skimage.segmentation.slic(img_as_float(img), **params, start_label=0)
    params         float64 [cases, 5]: n_segments, compactness, max_iter, enforce_connectivity, has_graph
    graph_x_<i>, graph_pos_<i>, graph_ei_<i>   the reference's graph (utils/dataloader.py:49-51 dtypes) for the
                   default-parameter cases (has_graph = 1)

plus ``merge`` / ``capped`` flags per case (connectivity relabelled a component / a flood fill hit max_size)
and the scikit-image, NumPy and SciPy versions.  Images of side 256 go to a second file so that each stays
under 1 MiB.
"""
import glob
import os
import sys
import types
import warnings

import numpy as np

warnings.filterwarnings("ignore")
REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

sys.modules.setdefault("torch", types.ModuleType("torch"))  # imported, never used, by the reference module
sys.path.insert(0, REF)
from utils.image_to_graph.image_to_graph_superpixel import image_to_graph_superpixel  # noqa: E402

import scipy  # noqa: E402
import skimage  # noqa: E402
from PIL import Image  # noqa: E402
from scipy import ndimage  # noqa: E402
from skimage.segmentation import slic  # noqa: E402
from skimage.segmentation.slic_superpixels import _get_grid_centroids  # noqa: E402
from skimage.util import img_as_float  # noqa: E402

PATHS = sorted(glob.glob(os.path.join(REF, "static", "*", "*.jpg")))


def resized(path, h, w):
    return np.array(Image.open(path).convert("RGB").resize((w, h)))


def flags(img, n, c, mi):
    """(merge, capped): does connectivity enforcement relabel a component, does a flood fill reach max_size."""
    raw = slic(img_as_float(img), n_segments=n, compactness=c, max_iter=mi, enforce_connectivity=False, start_label=0)
    k = _get_grid_centroids(img[None], n)[0].shape[0]
    seg = img.shape[0] * img.shape[1] / k
    min_size, max_size = int(0.5 * seg), int(3 * seg)
    merge = capped = False
    for lab in np.unique(raw):
        comp, nc = ndimage.label(raw == lab)
        sizes = np.bincount(comp.ravel())[1:]
        merge |= bool((sizes < min_size).any() or nc > 1)
        capped |= bool((sizes >= max_size).any())
    return merge, capped


def main():
    cases = []  # (img, n, compactness, max_iter, enforce, graph?)
    for R in (32, 64, 128):
        for p in PATHS:
            cases.append((resized(p, R, R), 100, 10, 10, True, True))
    for p in PATHS[:1] + PATHS[-1:]:
        cases.append((resized(p, 256, 256), 100, 10, 10, True, True))
    im128 = resized(PATHS[0], 128, 128)
    for n, c in ((25, 10), (400, 10), (100, 1), (100, 30)):
        cases.append((im128, n, c, 10, True, False))
    cases.append((resized(PATHS[1], 96, 160), 100, 10, 10, True, False))
    for p in PATHS[:2]:
        for R in (64, 128):
            img = resized(p, R, R)
            cases.append((img, 100, 10, 10, False, False))
            cases.append((img, 100, 10, 1, True, False))
            cases.append((img, 100, 10, 1, False, False))
    # a flood fill capped at max_size: search low compactness / few segments
    found = None
    for p in PATHS:
        img = resized(p, 64, 64)
        for n, c in ((10, 0.1), (20, 0.1), (10, 0.5), (50, 0.1), (30, 0.05)):
            if flags(img, n, c, 10)[1]:
                found = (img, n, c, 10, True, False)
                break
        if found:
            break
    if found:
        cases.append(found)
    small, big = {}, {}
    params, merge, capped = [], [], []
    for i, (img, n, c, mi, ec, graph) in enumerate(cases):
        d = big if img.shape[0] == 256 else small
        lab = slic(img_as_float(img), n_segments=n, compactness=c, max_iter=mi, enforce_connectivity=ec, start_label=0)
        d[f"img_{i}"] = img
        d[f"labels_{i}"] = lab.astype(np.int32)
        m, cp = flags(img, n, c, mi) if ec else (False, False)
        merge.append(m)
        capped.append(cp)
        params.append((n, c, mi, float(ec), float(graph)))
        if graph:
            x, pos, ei = image_to_graph_superpixel(Image.fromarray(img), resize_value=img.shape[0], n_segments=n,
                                                   compactness=c)
            d[f"graph_x_{i}"] = np.asarray(x, dtype=np.float32)
            d[f"graph_pos_{i}"] = np.asarray(pos, dtype=np.float32)
            d[f"graph_ei_{i}"] = np.asarray(ei).astype(np.int64)
        print(i, img.shape, n, c, mi, ec, "segments", len(np.unique(lab)), "merge", m, "capped", cp, flush=True)
    meta = dict(params=np.array(params, dtype=np.float64), merge=np.array(merge), capped=np.array(capped),
                versions=np.array([skimage.__version__, np.__version__, scipy.__version__]))
    np.savez_compressed(os.path.join(OUT, "g10_superpixel.npz"), **small, **meta)
    np.savez_compressed(os.path.join(OUT, "g10_superpixel_256.npz"), **big)


if __name__ == "__main__":
    main()
