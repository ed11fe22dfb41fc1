"""The region descriptor of DESIGN K26 written down once, for the tests of csrc/region_descriptor.hip.

Per region: exact integer sums (NumPy int64 / uint64 reductions over the region's pixels), then the 16 columns from Python
integers and floats.  Every expression below is the kernel's, in its operand order: the integer products and differences are
formed exactly (Python integers), ``float(int)`` and the C cast both round to nearest, and each division and ``math.sqrt`` is one
correctly rounded double operation, so both sides round alike and the float32 results can be compared bit for bit.
"""
import math

import numpy as np

DIM = 16
COLUMNS = ("mean_r", "mean_g", "mean_b", "std_r", "std_g", "std_b", "area", "bbox_height", "bbox_width", "spread_y", "spread_x",
           "box_fill", "boundary", "texture_r", "texture_g", "texture_b")
SQRT_COLUMNS = (3, 4, 5, 9, 10)
MAX_NODES, MAX_PIXELS = 512, 65536


def _segment_sums(order, starts, values):
    """int64 sum of ``values`` (any integer dtype) per run of the sorted pixel list"""
    return np.add.reduceat(values.astype(np.int64)[order], starts)


def region_sums(img: np.ndarray, lab: np.ndarray) -> dict:
    """The integers of every region, dense index = rank among the labels present (``np.unique``)."""
    H, W = lab.shape
    flat = lab.reshape(-1).astype(np.int64)
    uniq, inv = np.unique(flat, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(inv[order]) != 0])
    v = img.reshape(-1, 3).astype(np.int64)
    yy, xx = np.divmod(np.arange(H * W, dtype=np.int64), W)
    out = {"n": _segment_sums(order, starts, np.ones(H * W, np.int64)),
           "S": np.stack([_segment_sums(order, starts, v[:, c]) for c in range(3)], 1),
           "Q": np.stack([_segment_sums(order, starts, v[:, c] * v[:, c]) for c in range(3)], 1),
           "Sy": _segment_sums(order, starts, yy), "Sx": _segment_sums(order, starts, xx),
           "Syy": _segment_sums(order, starts, yy * yy), "Sxx": _segment_sums(order, starts, xx * xx),
           "ymin": np.minimum.reduceat(yy[order], starts), "ymax": np.maximum.reduceat(yy[order], starts),
           "xmin": np.minimum.reduceat(xx[order], starts), "xmax": np.maximum.reduceat(xx[order], starts)}
    # boundary pixels: a 4-neighbour inside the image with another label
    edge = np.zeros((H, W), bool)
    edge[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    edge[:, 1:] |= lab[:, 1:] != lab[:, :-1]
    edge[:-1, :] |= lab[:-1, :] != lab[1:, :]
    edge[1:, :] |= lab[1:, :] != lab[:-1, :]
    out["nb"] = _segment_sums(order, starts, edge.reshape(-1))
    # pixel pairs (p, q), q right of or below p, both in the region: credited to p
    im = img.astype(np.int64)
    pair = np.zeros((H, W), np.int64)
    diff = np.zeros((H, W, 3), np.int64)
    same_r = lab[:, :-1] == lab[:, 1:]
    pair[:, :-1] += same_r
    diff[:, :-1] += np.abs(im[:, :-1] - im[:, 1:]) * same_r[..., None]
    same_d = lab[:-1, :] == lab[1:, :]
    pair[:-1, :] += same_d
    diff[:-1, :] += np.abs(im[:-1, :] - im[1:, :]) * same_d[..., None]
    out["m"] = _segment_sums(order, starts, pair.reshape(-1))
    out["T"] = np.stack([_segment_sums(order, starts, diff[..., c].reshape(-1)) for c in range(3)], 1)
    out["labels"] = uniq
    return out


def descriptor_rows(img: np.ndarray, lab: np.ndarray) -> np.ndarray:
    """float32 [regions, 16] of one image whose labels all lie in [0, H W)"""
    H, W = lab.shape
    s = region_sums(img, lab)
    rows = np.zeros((len(s["n"]), DIM), np.float32)
    for i in range(len(s["n"])):
        n = int(s["n"][i])
        hgt, wid = int(s["ymax"][i] - s["ymin"][i] + 1), int(s["xmax"][i] - s["xmin"][i] + 1)
        m = int(s["m"][i])
        row = [0.0] * DIM
        for c in range(3):
            S, Q, T = int(s["S"][i, c]), int(s["Q"][i, c]), int(s["T"][i, c])
            row[c] = (S / 255.0) / n
            row[3 + c] = math.sqrt(float(n * Q - S * S)) / (255.0 * n)
            row[13 + c] = (T / 255.0) / m if m else 0.0
        Sy, Sx, Syy, Sxx = int(s["Sy"][i]), int(s["Sx"][i]), int(s["Syy"][i]), int(s["Sxx"][i])
        row[6] = float(n) / float(H * W)
        row[7] = float(hgt) / float(H)
        row[8] = float(wid) / float(W)
        row[9] = math.sqrt(float(n * Syy - Sy * Sy)) / (float(n) * float(H))
        row[10] = math.sqrt(float(n * Sxx - Sx * Sx)) / (float(n) * float(W))
        row[11] = float(n) / (float(hgt) * float(wid))
        row[12] = float(int(s["nb"][i])) / float(n)
        rows[i] = np.array(row, np.float64).astype(np.float32)
    return rows


def region_descriptors(img: np.ndarray, lab: np.ndarray, node_capacity: int = MAX_NODES):
    """What the kernel leaves for one image: ``(desc float32 [node_capacity, 16], counts int32 [3])`` with counts = (distinct labels
    inside [0, H W), bad-label flag, overflow flag); a flagged image is all zeros, rows behind the region count are zeros."""
    H, W = lab.shape
    valid = (lab >= 0) & (lab < H * W)
    regions = len(np.unique(lab[valid]))
    bad, overflow = int(not valid.all()), int(regions > node_capacity)
    desc = np.zeros((node_capacity, DIM), np.float32)
    if not bad and not overflow:
        desc[:regions] = descriptor_rows(img, lab)
    return desc, np.array([regions, bad, overflow], np.int32)


def region_descriptors_batch(imgs, labs, node_capacity: int = MAX_NODES):
    pairs = [region_descriptors(i, l, node_capacity) for i, l in zip(imgs, labs)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
