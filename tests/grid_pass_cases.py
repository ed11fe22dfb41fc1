"""Case builders and float64 CPU references of the tests that push the persistent-grid kernels beyond their first grid pass
(tests/test_gpu_grid_passes_xty.py, tests/test_gpu_grid_passes_rows.py, tests/test_gpu_grid_passes_topology.py).  No GPU here:
every size is a formula in the compute-unit count, which the GPU tests read from the device and hand in.

Integer cases: operands drawn from {-2 .. 2} and stored as fp32.  A product of two of them is an integer of magnitude <= 4 and a
sum of ``rows`` products stays below ``4 rows``; while that is below 2^24 every intermediate of an fp32 (FMA) accumulation IN ANY
ORDER is an exactly representable integer, so the kernel's result must have the BITS of the float64 result cast to fp32.  A
stale, dropped, repeated or mispaired row tile changes an integer.
"""
import torch

U = 2.0 ** -24
RPW = 32  # rows of one xty tile (one trip of one worker)


def ints(rows: int, cols: int, seed: int) -> torch.Tensor:
    """fp32 [rows, cols] of seeded integers from {-2 .. 2}."""
    assert 4 * rows < 2 ** 24, "sums of products of {-2..2} must stay exactly representable in fp32"
    return torch.randint(-2, 3, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


def normals(rows: int, cols: int, seed: int) -> torch.Tensor:
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def xty_rows(first_pass_workers: int) -> int:
    """Two full passes of every worker, five workers on a third trip, and a ragged last tile of 7 rows."""
    return 2 * first_pass_workers * RPW + 5 * RPW + 7


def colsum_rows(cus: int) -> int:
    """colsum_pair: 8 x CUs waves of 16 rows a trip; four full passes, five waves on a fifth trip, 7 ragged rows."""
    return 8 * cus * 16 * 4 + 16 * 5 + 7


def xty_ref(a: torch.Tensor, b: torch.Tensor):
    """float64 (A^T B [M, K], column sums of A [M])."""
    a64, b64 = a.double(), b.double()
    return a64.t() @ b64, a64.sum(0)


def xty_bounds(a: torch.Tensor, b: torch.Tensor):
    """First-order bound of a recursive fp32 sum of ``rows`` terms in any order, elementwise:
    ``rows 2^-24 (|A|^T |B|)`` for the product and ``rows 2^-24 sum |A|`` for the column sums."""
    rows = a.size(0)
    a64, b64 = a.double().abs(), b.double().abs()
    return rows * U * (a64.t() @ b64), rows * U * a64.sum(0)


def in_wider(t: torch.Tensor, left: int, right: int, seed: int) -> torch.Tensor:
    """``t`` as the columns [left, left + width) of a wider random table (its neighbours are NOT zero: a loader that strays
    across the slice's edge adds them)."""
    wide = normals(t.size(0), left + t.size(1) + right, seed)
    wide[:, left:left + t.size(1)] = t
    return wide


# ------------------------------------------------------------------------------------------------------------ row walkers
def row_pass_stride(cus: int, lanes_per_row: int) -> int:
    """Rows one trip of for_rows_two_in_flight's capped grid covers: 16 x CUs blocks of 256 / lpr rows."""
    return 16 * cus * (256 // lanes_per_row)


def row_pass_rows(cus: int, lanes_per_row: int) -> int:
    """The two-in-flight loop body runs twice (rows r, r + s, r + 2s, r + 3s), half the lanes' rows then meet the tail, 3 ragged."""
    s = row_pass_stride(cus, lanes_per_row)
    return 3 * s + s // 2 + 3


def lanes_for(width: int) -> int:
    lanes = 1
    while lanes * 4 < width:
        lanes *= 2
    return lanes


def random_index(n: int, e: int, seed: int, last_owns_rows: bool = True) -> torch.Tensor:
    index = torch.randint(0, n, (e,), generator=torch.Generator().manual_seed(seed))
    if last_owns_rows:
        index[-3:] = n - 1
    return index


def scatter_sum_ref(src: torch.Tensor, index: torch.Tensor, n: int) -> torch.Tensor:
    """float64 index_add_ of integer data, cast to fp32 (exact)."""
    out = torch.zeros(n, src.size(1), dtype=torch.float64)
    out.index_add_(0, index.long(), src.double())
    return out.float()


def attention_bars(src: torch.Tensor, scores: torch.Tensor, index: torch.Tensor, n: int, grad_out=None) -> dict:
    """segment_softmax_cases.bars (forward, saved_z, alpha, with ``grad_out`` grad_src and grad_score, and the reference tuple
    under "ref") for finite scores, with the per-destination Python loops replaced by scatter_reduce / index_add_ in float64 -
    the same formulas and constants (c_v = 2 deg_v + 2 dmax_v + 12); tests/test_grid_pass_cases_host.py holds the two against
    each other.  With ``grad_out`` also "want_src" / "want_score": segment_softmax_cases.ref_attention_backward."""
    idx, x, s = index.long(), src.double(), scores.double().reshape(-1)
    deg = torch.bincount(idx, minlength=n).double()
    m = torch.full((n,), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amax", include_self=True)
    m = torch.where(deg > 0, m, torch.zeros((), dtype=torch.float64))
    e = torch.exp(s - m[idx])
    z = torch.zeros(n, dtype=torch.float64).index_add_(0, idx, e)
    alpha = e / z[idx]
    zs = torch.where(deg > 0, z, torch.ones((), dtype=torch.float64))[:, None]
    out = torch.zeros(n, x.size(1), dtype=torch.float64).index_add_(0, idx, e[:, None] * x) / zs
    wabs = torch.zeros(n, x.size(1), dtype=torch.float64).index_add_(0, idx, e[:, None] * x.abs()) / zs
    dmax = torch.zeros(n, dtype=torch.float64).scatter_reduce(0, idx, (s - m[idx]).abs(), "amax", include_self=True)
    c = 2 * deg + 2 * dmax + 12
    b = {"forward": c[:, None] * U * wabs, "saved_z": (deg + 2 * dmax + 8) * U * z, "alpha": c[idx] * U * alpha,
         "ref": (out, alpha, m, z)}
    if grad_out is not None:
        g = grad_out.double()[idx]
        b["grad_src"] = c[idx][:, None] * U * (alpha[:, None] * g).abs()
        b["grad_score"] = (c[idx] + src.size(1)) * U * alpha * (g.abs() * (x.abs() + wabs[idx])).sum(1)
        b["want_src"], b["want_score"] = alpha[:, None] * g, alpha * (g * (x - out[idx])).sum(1)
    return b


def max_first_row_wins(src: torch.Tensor, index: torch.Tensor, n: int):
    """Vectorised (max [n, D] in src's dtype, argmax int64 [n, D]): the maximum per (destination, column) through
    scatter_reduce(amax), the winner = the LOWEST row that holds it (scatter_reduce(amin) over the row numbers of the hits);
    0 / -1 for a destination without rows.  For inputs without NaNs and without a -0.0 this is segment_reduce_cases.ref_max
    without its per-destination loop (tests/test_grid_pass_cases_host.py holds the two against each other)."""
    index = index.long()
    e, d = src.shape
    idx = index[:, None].expand(e, d)
    top = torch.full((n, d), float("-inf"), dtype=src.dtype).scatter_reduce(0, idx, src, "amax", include_self=True)
    rows = torch.arange(e)[:, None].expand(e, d)
    cand = torch.where(src == top[index], rows, torch.full_like(rows, e))
    arg = torch.full((n, d), e, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin", include_self=True)
    empty = arg == e
    return torch.where(empty, torch.zeros((), dtype=src.dtype), top), torch.where(empty, torch.full_like(arg, -1), arg)
