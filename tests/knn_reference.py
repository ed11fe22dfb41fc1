"""Brute-force NumPy reference of the k-nearest-neighbour edges (DESIGN K24), exact to the bit: the definition in
``include/gnc_hip.h`` spelled with float32 arrays.  Shared by the host and the GPU tests; nothing here needs a GPU."""
import numpy as np

NAN_FIELD = np.uint32(0xFFFFFFFF)


def distance_fields(feat: np.ndarray) -> np.ndarray:
    """uint32 [n, n]: the bits of d(v, u) = sum_c (f_v[c] - f_u[c])^2, accumulated in float32 with c ascending from +0.0 (one
    rounding per subtract, multiply and add - NumPy never fuses), a NaN replaced by the largest field."""
    f = np.ascontiguousarray(feat, dtype=np.float32)
    n, dim = f.shape
    d = np.zeros((n, n), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(dim):
            t = f[:, None, c] - f[None, :, c]
            d = d + t * t
    assert d.dtype == np.float32
    field = d.view(np.uint32).copy()
    field[np.isnan(d)] = NAN_FIELD
    return field


def knn_one_graph(feat: np.ndarray, k: int, loop: bool = False):
    """``(neighbours int64 [n, k], fields uint32 [n, k], keys uint64 [n, n])`` of ONE graph: row v holds the local ids and the
    distance fields of the k smallest keys ``field << 32 | u``; a slot without a candidate holds -1 and the bits of +inf.
    ``keys`` has the excluded diagonal at the largest uint64."""
    field = distance_fields(feat)
    n = field.shape[0]
    keys = (field.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    if not loop:
        keys[np.arange(n), np.arange(n)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(keys, axis=1, kind="stable")[:, :k]
    picked = np.take_along_axis(keys, order, axis=1)
    nbr = np.full((n, k), -1, dtype=np.int64)
    fld = np.full((n, k), 0x7F800000, dtype=np.uint32)
    have = min(k, n if loop else n - 1)
    nbr[:, :have] = order[:, :have]
    fld[:, :have] = (picked[:, :have] >> np.uint64(32)).astype(np.uint32)
    return nbr, fld, keys


def knn_graph(feat: np.ndarray, k: int, graph_ptr=None, loop: bool = False):
    """``(edge_index int64 [2, k N], dist_bits uint32 [k N])`` of a batch: slot ``v k + j`` = (sender, receiver v) with global ids,
    -1 / -1 / +inf where a graph has no j-th candidate."""
    feat = np.asarray(feat, dtype=np.float32)
    N = feat.shape[0]
    ptr = [0, N] if graph_ptr is None else [int(p) for p in graph_ptr]
    ei = np.full((2, k * N), -1, dtype=np.int64)
    bits = np.full(k * N, 0x7F800000, dtype=np.uint32)
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b == a:
            continue
        nbr, fld, _ = knn_one_graph(feat[a:b], k, loop)
        recv = np.repeat(np.arange(a, b, dtype=np.int64), k).reshape(b - a, k)
        ok = nbr >= 0
        ei[0, a * k:b * k] = np.where(ok, nbr + a, -1).reshape(-1)
        ei[1, a * k:b * k] = np.where(ok, recv, -1).reshape(-1)
        bits[a * k:b * k] = fld.reshape(-1)
    return ei, bits


def rows_cut_inside_a_tie(feat: np.ndarray, k: int, loop: bool = False) -> int:
    """Rows whose k-th and (k+1)-th candidates have the SAME distance field: there the index half of the key decides the edge."""
    _, _, keys = knn_one_graph(feat, k, loop)
    s = np.sort(keys, axis=1)
    if s.shape[1] <= k:
        return 0
    real = s[:, k] != np.uint64(0xFFFFFFFFFFFFFFFF)
    return int(np.sum(real & ((s[:, k - 1] >> np.uint64(32)) == (s[:, k] >> np.uint64(32)))))


def integer_grid(side: int = 9) -> np.ndarray:
    """float32 [side^2, 2]: the points (i, j) of an integer grid - every row has tied distances."""
    ii, jj = np.mgrid[0:side, 0:side]
    return np.stack([ii.reshape(-1), jj.reshape(-1)], axis=1).astype(np.float32)
