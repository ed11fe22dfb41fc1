"""Sequential SLIC superpixels on the CPU: scikit-image 0.18.3 ``slic(img_as_float(img), ...)`` for one 2-D uint8 RGB
image, restated in NumPy from the published algorithm as the header of ``graphnet_classifier_amd/csrc/superpixel.hip``
documents it (Lab conversion, sigma = 0, no mask, unit spacing, SLIC not SLIC-zero).

It is the reference for the device SLIC at shapes the fixtures do not reach.  Its licence is
``tests/test_slic_oracle_host.py``: all 44 label images of ``tests/golden/g10_superpixel*.npz`` (scikit-image's own
output) are reproduced bit for bit.  It shares no structure with the kernel: the centres are visited one after the
other in index order, each over its whole window, against one distance map; there are no tiles, no candidate lists and
no bounding boxes.

float64 throughout and no fused multiply-add: every product and sum is its own NumPy operation, and the colour matrix
is written out as ``r*m0 + g*m1 + b*m2`` (a BLAS product may contract or reorder it).

    python -m oracle.slic_oracle        # per-fixture mismatch counts and timing
"""
import time

import numpy as np

DBL_MAX = np.finfo(np.float64).max

# skimage.color.colorconv: xyz_from_rgb and the D65 / 2-degree observer white point
XYZ_FROM_RGB = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
XYZ_REF_WHITE = (0.95047, 1.0, 1.08883)


def gamma_table() -> np.ndarray:
    """rgb2xyz's sRGB gamma of the 256 values ``u * (1 / 255)`` (img_as_float of uint8)."""
    v = np.multiply(np.arange(256), 1.0 / 255, dtype=np.float64)
    out = v.copy()
    hi = v > 0.04045
    out[hi] = np.power((v[hi] + 0.055) / 1.055, 2.4)
    out[~hi] /= 12.92
    return out


def rgb2lab_u8(img_u8: np.ndarray) -> np.ndarray:
    """float64 [H, W, 3]: rgb2lab(img_as_float(img_u8))."""
    lin = gamma_table()[img_u8]
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    t = []
    for (m0, m1, m2), white in zip(XYZ_FROM_RGB, XYZ_REF_WHITE):
        v = (r * m0 + g * m1 + b * m2) / white
        hi = v > 0.008856
        f = np.empty_like(v)
        f[hi] = np.cbrt(v[hi])
        f[~hi] = 7.787 * v[~hi] + 16.0 / 116.0
        t.append(f)
    x, y, z = t
    return np.stack([(116.0 * y) - 16.0, 500.0 * (x - y), 200.0 * (y - z)], axis=-1)


def regular_grid(shape, n_points):
    """skimage.util.regular_grid: one slice per axis that picks about ``n_points`` evenly spaced points of ``shape``."""
    shape = np.asarray(shape)
    ndim = len(shape)
    unsort = np.argsort(np.argsort(shape))
    dims = np.sort(shape)
    space = float(np.prod(shape))
    if space <= n_points:
        return (slice(None),) * ndim
    steps = np.full(ndim, (space / n_points) ** (1.0 / ndim), dtype=np.float64)
    if (dims < steps).any():  # a short axis: it keeps every point, the longer ones share the rest
        for d in range(ndim):
            steps[d] = dims[d]
            space = float(np.prod(dims[d + 1:]))
            steps[d + 1:] = (space / n_points) ** (1.0 / (ndim - d - 1))
            if (dims >= steps).all():
                break
    starts = (steps // 2).astype(int)
    steps = np.round(steps).astype(int)
    slices = [slice(int(a), None, int(s)) for a, s in zip(starts, steps)]
    return tuple(slices[i] for i in unsort)


def _steps(slices):
    return [int(s.step) if s.step is not None else 1 for s in slices]


def seed_centres(H: int, W: int, n_segments: int):
    """(float64 [K, 2] centre (y, x) in index order, spatial step = max of the seed grid's steps)."""
    slices = regular_grid((1, H, W), n_segments)
    grid = np.mgrid[:1, :H, :W][(slice(None),) + slices]  # [3, nz, ny, nx]
    yx = np.stack([grid[1].ravel(), grid[2].ravel()], axis=-1).astype(np.float64)
    return yx, max(_steps(slices))


def _assign(lab, centres, alive, near, wy, wx, sw):
    """One pass of the centre loop; returns whether any pixel took a centre."""
    H, W = near.shape
    dist = np.full((H, W), DBL_MAX)
    change = False
    for k in range(len(centres)):
        if not alive[k]:
            continue
        cy, cx, cl, ca, cb = centres[k]
        y0, y1 = int(max(cy - 2 * wy, 0)), int(min(cy + 2 * wy + 1, H))
        x0, x1 = int(max(cx - 2 * wx, 0)), int(min(cx + 2 * wx + 1, W))
        if y0 >= y1 or x0 >= x1:
            continue
        dy = (cy - np.arange(y0, y1, dtype=np.float64)) ** 2
        dx = (cx - np.arange(x0, x1, dtype=np.float64)) ** 2
        d = (dy[:, None] + dx[None, :]) * sw
        win = lab[y0:y1, x0:x1]
        col = (win[..., 0] - cl) ** 2
        col = col + (win[..., 1] - ca) ** 2
        col = col + (win[..., 2] - cb) ** 2
        d = d + col
        cur = dist[y0:y1, x0:x1]
        take = cur > d  # strict: a tie stays with the lower centre index
        if take.any():
            cur[take] = d[take]
            near[y0:y1, x0:x1][take] = k
            change = True
    return change


def _update(lab, near, centres, alive):
    """Centres move to the mean of their pixels, sums in raster order; returns whether any centre is empty."""
    K = len(centres)
    flat = near.ravel()
    owned = flat >= 0  # a pixel no window has covered yet belongs to no centre
    idx = flat[owned]
    yy, xx = np.divmod(np.flatnonzero(owned), near.shape[1])
    cnt = np.bincount(idx, minlength=K)
    sums = [np.bincount(idx, weights=v, minlength=K)  # bincount adds in input order: the raster order
            for v in (yy.astype(np.float64), xx.astype(np.float64), lab[..., 0].ravel()[owned],
                      lab[..., 1].ravel()[owned], lab[..., 2].ravel()[owned])]
    full = cnt > 0
    for j, s in enumerate(sums):
        centres[full, j] = s[full] / cnt[full]
    alive[:] = full  # 0 / 0 = NaN in the sequential code, and no distance to NaN is ever smaller
    return not bool(full.all())


def enforce_label_connectivity(segments: np.ndarray, min_size: int, max_size: int, start_label: int = 0):
    """_enforce_label_connectivity_cython as a plain breadth-first fill; returns (int32 labels, number of labels)."""
    H, W = segments.shape
    seg = segments.ravel().tolist()
    unset = start_label - 1
    out = [unset] * (H * W)
    cur = start_label
    for p0 in range(H * W):
        label = seg[p0]
        if label == unset or out[p0] >= start_label:
            continue
        adjacent = 0
        out[p0] = cur
        queue = [p0]
        visited = 0
        while visited < len(queue) < max_size:
            q = queue[visited]
            qy, qx = divmod(q, W)
            for r, inside in ((q + 1, qx + 1 < W), (q - 1, qx >= 1), (q + W, qy + 1 < H), (q - W, qy >= 1)):
                if not inside:
                    continue
                o = out[r]
                if seg[r] == label and o == unset:
                    out[r] = cur
                    queue.append(r)
                    if len(queue) >= max_size:
                        break
                elif o >= start_label and o != cur:
                    adjacent = o
            visited += 1
        if len(queue) < min_size:
            for q in queue:
                out[q] = adjacent
        else:
            cur += 1
    return np.asarray(out, dtype=np.int32).reshape(H, W), cur - start_label


def slic(img_u8, n_segments=100, compactness=10.0, max_iter=10, enforce_connectivity=True, min_size_factor=0.5,
         max_size_factor=3.0, start_label=0):
    """(int32 labels [H, W], info) with info = dict(K: seeded centres, emptied: a centre had no pixel after some update -
    the one behind the last assignment included, which the sequential code runs and nobody reads -, n_labels: labels
    handed out, K without connectivity enforcement)."""
    img_u8 = np.asarray(img_u8)
    if img_u8.dtype != np.uint8 or img_u8.ndim != 3 or img_u8.shape[2] != 3:
        raise ValueError("slic oracle: expected a uint8 RGB image [H, W, 3]")
    H, W = img_u8.shape[:2]
    lab = rgb2lab_u8(img_u8) * (1.0 / compactness)
    yx, step = seed_centres(H, W, n_segments)
    K = len(yx)
    centres = np.zeros((K, 5))  # y, x, L, a, b
    centres[:, :2] = yx
    alive = np.ones(K, dtype=bool)
    _, wy, wx = _steps(regular_grid((1, H, W), K))  # the windows follow the grid of the actual centre count
    sw = 1.0 / (step * step)
    near = np.full((H, W), -1, dtype=np.int64)
    emptied = False
    for _ in range(max_iter):
        if not _assign(lab, centres, alive, near, wy, wx, sw):
            break
        emptied |= _update(lab, near, centres, alive)
    info = dict(K=K, emptied=emptied, n_labels=K)
    if not enforce_connectivity:
        return (near + start_label).astype(np.int32), info
    segment_size = H * W / K
    labels, info["n_labels"] = enforce_label_connectivity(
        near + start_label, int(min_size_factor * segment_size), int(max_size_factor * segment_size), start_label)
    return labels, info


def main():
    from tests.test_superpixel_golden import CASES
    total = 0.0
    bad = 0
    for i, img, ref, (n, c, mi, ec), _ in CASES:
        t0 = time.perf_counter()
        labels, info = slic(img, n_segments=n, compactness=c, max_iter=mi, enforce_connectivity=ec)
        dt = time.perf_counter() - t0
        total += dt
        mism = int((labels != ref).sum())
        bad += mism != 0
        print(f"case {i:2d} {img.shape[0]:3d}x{img.shape[1]:<3d} n={n:3d} c={c:<4g} iter={mi:2d} conn={int(ec)} K={info['K']:3d} "
              f"labels={info['n_labels']:3d} emptied={int(info['emptied'])} mismatches={mism} of {ref.size}  {dt:.2f} s")
    print(f"{len(CASES) - bad} of {len(CASES)} fixtures bit for bit, {total:.1f} s")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
