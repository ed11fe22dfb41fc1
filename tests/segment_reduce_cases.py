"""Case builders and the float64 CPU reference of the mean / max neighbourhood aggregation (K18), shared by
tests/test_segment_reduce_host.py, tests/test_gpu_segment_reduce.py and tests/test_gpu_aggregation_model.py.  No GPU here.

The reference is plain torch on the CPU, one destination at a time: ``rows`` = the rows of ``src`` with ``index == v`` in
ascending row order.
  mean[v]   = float64 sum of ``src[rows]`` / len(rows), 0 for no rows;
  max[v, c] = the value of the LOWEST row among those that hold the column's maximum (so ``-0.0`` against ``+0.0`` keeps the
              first one's sign bit); a column with a NaN takes its first NaN row; 0 and argmax -1 for no rows;
  backwards = the chain rule of exactly that: ``grad_out[index[r]] / deg`` and ``grad_out[index[r], c]`` at the winner.
"""
import torch

# ---------------------------------------------------------------------------------------------------------------- reference


def _segments(index: torch.Tensor, num_nodes: int):
    """[rows of destination v, ascending] for v in range(num_nodes)."""
    index = index.long()
    order = torch.argsort(index, stable=True)
    counts = torch.bincount(index, minlength=num_nodes)
    return list(torch.split(order, counts.tolist()))


def degrees(index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    return torch.bincount(index.long(), minlength=num_nodes)


def ref_mean(src: torch.Tensor, index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """float64 [num_nodes, D]."""
    out = torch.zeros(num_nodes, src.size(1), dtype=torch.float64)
    for v, rows in enumerate(_segments(index, num_nodes)):
        if rows.numel():
            out[v] = src[rows].double().sum(0) / rows.numel()
    return out


def ref_abs_sum(src: torch.Tensor, index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """float64 [num_nodes, D]: sum of |src| per destination, the scale of the recursive-summation bound."""
    out = torch.zeros(num_nodes, src.size(1), dtype=torch.float64)
    out.index_add_(0, index.long(), src.double().abs())
    return out


def ref_max(src: torch.Tensor, index: torch.Tensor, num_nodes: int):
    """(max in the dtype of ``src`` - a maximum is one of its inputs, bit for bit -, argmax int64 [num_nodes, D])."""
    d = src.size(1)
    out = torch.zeros(num_nodes, d, dtype=src.dtype)
    arg = torch.full((num_nodes, d), -1, dtype=torch.int64)
    for v, rows in enumerate(_segments(index, num_nodes)):
        if not rows.numel():
            continue
        seg = src[rows]                                                         # [deg, D], rows ascending
        nan = torch.isnan(seg)
        top = torch.where(nan, torch.full_like(seg, float("-inf")), seg).max(0).values
        hit = torch.where(nan.any(0)[None, :], nan, seg == top[None, :])        # a NaN column: its NaN rows; else the maxima
        pos = torch.arange(rows.numel())[:, None].expand_as(hit)
        first = torch.where(hit, pos, torch.full_like(pos, rows.numel())).min(0).values
        out[v] = seg.gather(0, first[None, :])[0]
        arg[v] = rows[first]
    return out, arg


def ref_mean_backward(grad_out: torch.Tensor, index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """float64 [E, D]."""
    deg = degrees(index, num_nodes).double()
    return grad_out.double()[index.long()] / deg[index.long()][:, None]


def ref_max_backward(grad_out: torch.Tensor, index: torch.Tensor, argmax: torch.Tensor) -> torch.Tensor:
    """[E, D] in the dtype of ``grad_out``: ``grad_out`` at the winner, +0.0 elsewhere."""
    index = index.long()
    rows = torch.arange(index.numel())[:, None]
    return torch.where(argmax[index] == rows, grad_out[index], torch.zeros((), dtype=grad_out.dtype))


# ------------------------------------------------------------------------------------- stand-ins for the oracle's _scatter
# ``oracle.graphnet_oracle._scatter(edge_attr, col, dim_size)`` replaced through monkeypatch by these: differentiable (the
# float64 autograd reference) and in the dtype of their input (the fp32 oracle).

def oracle_scatter_mean(src: torch.Tensor, index: torch.Tensor, dim_size: int) -> torch.Tensor:
    out = src.new_zeros((dim_size, src.size(1)))
    out.index_add_(0, index.long(), src)
    return out / degrees(index, dim_size).clamp(min=1).to(src.dtype)[:, None]


MAX_GAPS: list = []  # filled by oracle_scatter_max while RECORD_GAPS is on: min (largest - second largest) of every call
RECORD_GAPS = False


def oracle_scatter_max(src: torch.Tensor, index: torch.Tensor, dim_size: int) -> torch.Tensor:
    with torch.no_grad():
        _, arg = ref_max(src.detach(), index, dim_size)
        if RECORD_GAPS:
            MAX_GAPS.append(min_top2_gap(src.detach(), index, dim_size))
    picked = src.gather(0, arg.clamp(min=0))  # differentiable: the gradient of a column goes to the row that won it
    return torch.where(arg >= 0, picked, src.new_zeros(()))


def min_top2_gap(src: torch.Tensor, index: torch.Tensor, num_nodes: int) -> float:
    """Smallest gap between the largest and the second-largest candidate over every (destination, column) with two or more."""
    best = float("inf")
    for rows in _segments(index, num_nodes):
        if rows.numel() >= 2:
            top2 = src[rows].topk(2, dim=0).values
            best = min(best, float((top2[0] - top2[1]).min()))
    return best


ORACLE_SCATTER = {"mean": oracle_scatter_mean, "max": oracle_scatter_max}

# -------------------------------------------------------------------------------------------------------------------- cases

SMALL_N, SMALL_E, HUB = 37, 211, 70
# destination degrees of the small regime: the unrolled-by-four loop (4, 5, 9, 70), its tail (1, 3, 5, 9, 70), the empty row (0)
SMALL_DEGREES = (0,) * 3 + (1,) * 6 + (3,) * 6 + (4,) * 8 + (5,) * 8 + (9,) * 5 + (HUB,)
SMALL_WIDTHS = (3, 8, 64, 128, 256)
# the chunk walker's corners: one lane per row (4), 64 lanes per row (256), lane groups with idle lanes (12, 100)
CHUNK_WIDTHS = (4, 12, 64, 100, 128, 256)


def small_index(seed: int = 0) -> torch.Tensor:
    """int64 [211] destinations in a shuffled (unsorted) order: 37 destinations with the degrees of SMALL_DEGREES, dealt to the
    node ids by a seeded permutation (so the empty rows and the hub sit anywhere)."""
    assert len(SMALL_DEGREES) == SMALL_N and sum(SMALL_DEGREES) == SMALL_E
    g = torch.Generator().manual_seed(seed)
    nodes = torch.randperm(SMALL_N, generator=g)
    index = torch.repeat_interleave(nodes, torch.tensor(SMALL_DEGREES))
    return index[torch.randperm(SMALL_E, generator=g)]


def values(rows: int, width: int, seed: int) -> torch.Tensor:
    return torch.randn(rows, width, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def chunk_index(num_nodes: int, seed: int = 1) -> torch.Tensor:
    """int64 [4 * num_nodes] random destinations (in-degrees 0 .. ~15), unsorted."""
    return torch.randint(0, num_nodes, (4 * num_nodes,), generator=torch.Generator().manual_seed(seed))


def hand_example():
    """5 destinations, 7 rows, 2 columns: destination 3 is empty, destination 1 holds a tie in column 0 (rows 1 and 4, the
    value 2.0) and -0.0 against +0.0 in column 1 (row 1 first), destination 4 has one row.
    Returns (src, index, mean, max, argmax) with the answers written out by hand."""
    index = torch.tensor([0, 1, 0, 2, 1, 4, 1])
    src = torch.tensor([[1.0, -1.0],    # -> 0
                        [2.0, -0.0],    # -> 1
                        [3.0, 5.0],     # -> 0
                        [-4.0, 0.5],    # -> 2
                        [2.0, 0.0],     # -> 1
                        [7.0, -7.0],    # -> 4
                        [-6.0, -3.0]])  # -> 1
    mean = torch.tensor([[2.0, 2.0], [-2.0 / 3.0, -1.0], [-4.0, 0.5], [0.0, 0.0], [7.0, -7.0]], dtype=torch.float64)
    mx = torch.tensor([[3.0, 5.0], [2.0, -0.0], [-4.0, 0.5], [0.0, 0.0], [7.0, -7.0]])
    arg = torch.tensor([[2, 2], [1, 1], [3, 3], [-1, -1], [5, 5]])
    return src, index, mean, mx, arg
