"""GPU, kernel level: the row and destination walkers of csrc/segment_csr.h and their users (scatter_gather.hip,
segment_reduce.hip, segment_softmax.hip) at sizes where a worker of the capped grid makes a second and a third trip:

  for_rows_two_in_flight (gather_rows, gather_rows_add, segment_reduce_backward; segment_softmax_backward keeps the same loop
  written out): rows = 3 s + s / 2 + 3 with s = 16 x CUs x 256 / lanes-per-row rows per grid trip - the two-in-flight body runs
  twice for some rows (r, r + s, then r + 2 s, r + 3 s), the others finish in the tail;
  grid-stride element loops (gather_rows scalar, edge_features, poison_if_flagged_, rows_div_degree_, the scalar
  segment_reduce_backward, segment_softmax_weights): two passes of the capped grid plus 1027 items;
  for_scalar_destinations: N = 2 x 64 x CUs + 5 destinations (one wave each; five waves on a third trip);
  for_chunk_destinations: N = 2 x 4096 x CUs + 64 x 5 + 1 (five waves on a third chunk and one last chunk of ONE destination).

Every size is derived from multi_processor_count, and every test asserts its trip-count premise before it launches.
Bars: gathers, integer sums, maxima and argmax are bit-exact; the float cases reuse the bounds of tests/test_gpu_segment_reduce.py
and tests/test_gpu_segment_softmax.py (tests/segment_softmax_cases.py) and print the share of the bound they use.
"""
import numpy as np
import pytest
import torch

from oracle import graphnet_oracle as O
from tests import grid_pass_cases as G
from tests import segment_reduce_cases as R
from tests import segment_softmax_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def native():
    from graphnet_classifier_amd import native as n
    n.load_library()
    return n


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _csr(index, n):
    from graphnet_classifier_amd.topology import DestinationCSR
    return DestinationCSR(index.to(DEV), n, torch.device(DEV))


def _within(err, bar, what):
    used = S.fraction(err, bar)
    print(f"{what}: uses {used:.3f} of its bar")
    assert used <= 1.0, what


def _two_in_flight_rows(width):
    """(rows, lanes per row) with the premise of the two-in-flight loop: more than three and fewer than four grid trips."""
    cus, lpr = _cus(), G.lanes_for(width)
    stride, rows = G.row_pass_stride(cus, lpr), G.row_pass_rows(cus, lpr)
    assert 3 * stride < rows < 4 * stride and stride == 16 * cus * (256 // lpr)
    return rows, lpr


def _ints8(rows, cols, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-2, 3, size=(rows, cols), dtype=np.int8))


# ---------------------------------------------------------------------------------------------- K2, the vector row pass
@pytest.mark.parametrize("add", [False, True], ids=["gather_rows", "gather_rows_add"])
@pytest.mark.parametrize("d", [4, 64, 200, 256])
def test_gather_rows_two_in_flight_loop_runs_twice_and_meets_its_tail(native, d, add):
    rows, lpr = _two_in_flight_rows(d)
    assert lpr == {4: 1, 64: 16, 200: 64, 256: 64}[d]
    n = 513
    table = G.normals(n, d, seed=d)
    idx = torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(d + 1), dtype=torch.int32)
    want = table[idx.long()]
    if add:
        addend = G.normals(rows, d, seed=d + 2)
        want += addend
        out = native.gather_rows_add(table.to(DEV), idx.to(DEV), addend.to(DEV))
    else:
        out = native.gather_rows(table.to(DEV), idx.to(DEV))
    assert torch.equal(out, want.to(DEV))


@pytest.mark.parametrize("add", [False, True], ids=["gather_rows", "gather_rows_add"])
def test_gather_rows_two_in_flight_on_strided_views(native, add):
    """Table, addend and output as 16-B aligned column slices of wider tensors (the vector kernel): the columns on both sides of
    the output keep their sentinel."""
    d = 64
    rows, _ = _two_in_flight_rows(d)
    lib = native.load_library()
    n = 513
    table_w = G.normals(n, d + 8, seed=1)
    idx = torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    table = table_w.to(DEV)[:, 4:4 + d]
    out_w = torch.full((rows, d + 12), -7.25, device=DEV)
    out = out_w[:, 8:8 + d]
    idx_dev = idx.to(DEV)
    want = table_w[:, 4:4 + d][idx.long()]
    assert table.stride(0) % 4 == 0 and table.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0
    if add:
        add_w = G.normals(rows, d + 4, seed=3)
        addend = add_w.to(DEV)[:, 4:4 + d]
        want = want + add_w[:, 4:4 + d]
        rc = lib.gnc_gather_rows_add_f32(table.data_ptr(), table.stride(0), idx_dev.data_ptr(), addend.data_ptr(), addend.stride(0),
                                         rows, d, out.data_ptr(), out.stride(0), native._stream(table))
    else:
        rc = lib.gnc_gather_rows_f32(table.data_ptr(), table.stride(0), idx_dev.data_ptr(), rows, d, out.data_ptr(), out.stride(0),
                                     native._stream(table))
    native._check(rc, "gather into a view")
    assert torch.equal(out, want.to(DEV))
    assert bool((out_w[:, :8] == -7.25).all()) and bool((out_w[:, 8 + d:] == -7.25).all())


# ------------------------------------------------------------------------ K18 / K21 backwards, the vector row pass at D = 256
def _backward_case():
    d = 256
    rows, lpr = _two_in_flight_rows(d)
    assert lpr == 64
    n = rows // 6
    index = G.random_index(n, rows, seed=5)
    return d, rows, n, index


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_segment_reduce_backward_two_in_flight(native, mode):
    d, rows, n, index = _backward_case()
    csr = _csr(index, n)
    grad = R.values(n, d, seed=6)
    if mode == "mean":
        got = native.segment_reduce_backward(grad.to(DEV), csr.col32, csr.rowptr, None, "mean")
        want = R.ref_mean_backward(grad, index, n)
        err = (got.cpu().double() - want).abs()
        print(f"mean backward: err / (2^-23 |want|) at most {float((err / (2.0 ** -23 * want.abs()).clamp(min=1e-300)).max()):.3f}")
        assert bool((err <= 2.0 ** -23 * want.abs()).all())
    else:
        src = R.values(rows, d, seed=7)
        _, r_arg = G.max_first_row_wins(src, index, n)
        got = native.segment_reduce_backward(grad.to(DEV), csr.col32, csr.rowptr, r_arg.int().to(DEV), "max")
        assert _bits(got.cpu(), R.ref_max_backward(grad, index, r_arg))


def test_segment_softmax_backward_two_in_flight(native):
    d, rows, n, index = _backward_case()
    csr = _csr(index, n)
    src, scores, grad = S.values(rows, d, seed=8), S.scores_for(rows, 3, seed=8), S.values(n, d, seed=9)
    out, saved = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), csr.rowptr, csr.perm, n)
    g_src, g_s = native.segment_softmax_backward(grad.to(DEV), src.to(DEV), scores.to(DEV), out, saved, csr.col32)
    b = G.attention_bars(src, scores, index, n, grad)  # the bars and reference of segment_softmax_cases, without its loops
    _within((g_src.cpu().double() - b["want_src"]).abs(), b["grad_src"], f"{rows} rows, D={d} grad_src")
    _within((g_s.cpu().double() - b["want_score"]).abs(), b["grad_score"], f"{rows} rows, D={d} grad_score")


# ------------------------------------------------------------------------------------------- grid-stride element loops
def _two_passes_and_a_tail(per_cu):
    """Items for a grid capped at per_cu x CUs threads: two full passes and 1027 more."""
    cap = per_cu * _cus()
    items = 2 * cap + 1027
    assert 2 * cap < items < 3 * cap
    return items


def test_gather_rows_scalar_third_trip(native):
    items = _two_passes_and_a_tail(4096)
    rows = -(-items // 3)
    assert rows * 3 > 2 * 4096 * _cus()
    table = G.normals(513, 3, seed=11)
    idx = torch.randint(0, 513, (rows,), generator=torch.Generator().manual_seed(12), dtype=torch.int32)
    assert torch.equal(native.gather_rows(table.to(DEV), idx.to(DEV)).cpu(), table[idx.long()])
    addend = G.normals(rows, 3, seed=13)
    assert torch.equal(native.gather_rows_add(table.to(DEV), idx.to(DEV), addend.to(DEV)).cpu(), table[idx.long()] + addend)


@pytest.mark.parametrize("space_dim", [2, 3])
def test_edge_features_third_trip(native, space_dim):
    e = _two_passes_and_a_tail(4096)
    rng = np.random.default_rng(space_dim)
    n = 211
    pos = torch.from_numpy((rng.random((n, space_dim)) * 32).astype(np.float32))
    ei = torch.from_numpy(rng.integers(0, n, size=(2, e)).astype(np.int64))
    out = native.edge_features(pos.to(DEV), ei[0].int().to(DEV), ei[1].int().to(DEV)).cpu()
    ref = O.edge_features(pos, ei)
    err = float((out.double() - ref.double()).abs().max())
    print(f"edge_features E={e} space_dim={space_dim}: distance column off by at most {err:.3e} (bar 4e-6)")
    assert err <= 4e-6  # |.|-sum order may differ for space_dim == 3
    assert torch.equal(out[:, :space_dim], ref[:, :space_dim])


def test_poison_if_flagged_third_trip(native):
    count = _two_passes_and_a_tail(1024)
    out = torch.arange(count, dtype=torch.float32, device=DEV)
    flags = torch.zeros(3, dtype=torch.int32, device=DEV)
    native.poison_if_flagged_(out, flags)
    assert torch.equal(out, torch.arange(count, dtype=torch.float32, device=DEV))  # flag clear: nothing is touched
    flags[1] = 1
    native.poison_if_flagged_(out, flags)
    assert bool(torch.isnan(out).all())


def test_rows_div_degree_third_trip(native):
    """One item = four columns of one row; D = 4: one item per destination."""
    n = _two_passes_and_a_tail(4096)
    index = G.random_index(n, n + n // 2, seed=14)
    deg = R.degrees(index, n)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).int()
    table = G.normals(n, 4, seed=15)
    got = native.rows_div_degree_(table.to(DEV), rowptr.to(DEV)).cpu()
    assert bool((deg == 0).any()) and _bits(got[deg == 0], table[deg == 0])  # rows of degree 0 are left alone
    want = table.double() / deg.clamp(min=1).double()[:, None]
    err = (got.double() - want).abs()
    print(f"rows_div_degree N={n}: err / (2^-24 |want|) at most {float((err / (U * want.abs()).clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= U * want.abs()).all())  # one correctly rounded division


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_segment_reduce_backward_scalar_third_trip(native, mode):
    items = _two_passes_and_a_tail(4096)
    d = 3
    rows = -(-items // d)
    assert rows * d > 2 * 4096 * _cus()
    n = rows // 6
    index = G.random_index(n, rows, seed=16)
    csr = _csr(index, n)
    grad = R.values(n, d, seed=17)
    if mode == "mean":
        got = native.segment_reduce_backward(grad.to(DEV), csr.col32, csr.rowptr, None, "mean")
        want = R.ref_mean_backward(grad, index, n)
        assert bool(((got.cpu().double() - want).abs() <= 2.0 ** -23 * want.abs()).all())
    else:
        _, r_arg = G.max_first_row_wins(R.values(rows, d, seed=18), index, n)
        got = native.segment_reduce_backward(grad.to(DEV), csr.col32, csr.rowptr, r_arg.int().to(DEV), "max")
        assert _bits(got.cpu(), R.ref_max_backward(grad, index, r_arg))


def test_segment_softmax_weights_third_trip(native):
    rows = _two_passes_and_a_tail(4096)
    n = rows // 4
    index = G.random_index(n, rows, seed=19)
    scores = S.scores_for(rows, 3, seed=19)
    b = G.attention_bars(torch.zeros(rows, 1), scores, index, n)
    _, r_alpha, r_m, r_z = b["ref"]
    saved = torch.stack([r_m.float(), r_z.float()], dim=1).contiguous()  # m is one of the scores: exact; Z rounded once
    assert torch.equal(saved[:, 0].double(), r_m)
    alpha = native.segment_softmax_weights(scores.to(DEV), saved.to(DEV), index.int().to(DEV))
    _within((alpha.cpu().double() - r_alpha).abs(), b["alpha"], f"weights of {rows} rows")


# ----------------------------------------------------------------------------------------- for_scalar_destinations
def _scalar_walker_case():
    cus = _cus()
    n = 2 * 64 * cus + 5
    assert n > 2 * 64 * cus  # one wave per destination, 64 x CUs waves: five of them take a third destination
    return n, G.random_index(n, 4 * n, seed=21)


@pytest.mark.parametrize("d", [3, 260])
def test_scatter_sum_scalar_walker_third_trip_is_exact_on_integers(native, d):
    n, index = _scalar_walker_case()
    src = G.ints(index.numel(), d, seed=d)
    csr = _csr(index, n)
    out = native.scatter_sum_csr(src.to(DEV), csr.rowptr, csr.perm, n)
    assert _bits(out.cpu(), G.scatter_sum_ref(src, index, n))


def test_segment_max_scalar_walker_third_trip_on_an_offset_view(native):
    """ld_src = 72 != D = 64 and a base 4 bytes past a 16-byte boundary: the scalar kernel."""
    n, index = _scalar_walker_case()
    wide = R.values(index.numel(), 72, seed=22)
    view = wide.to(DEV)[:, 1:65]
    assert view.stride(0) == 72 and view.data_ptr() % 16 == 4
    csr = _csr(index, n)
    r_max, r_arg = G.max_first_row_wins(wide[:, 1:65].contiguous(), index, n)
    mx, arg = native.segment_reduce_csr(view, csr.rowptr, csr.perm, n, "max", with_argmax=True)
    assert _bits(mx.cpu(), r_max) and torch.equal(arg.long().cpu(), r_arg)
    assert bool((r_arg[n - 1] >= 0).all()) and bool((r_arg == -1).any())
    # the mean through the same walker: the bound of tests/test_gpu_segment_reduce.py, its sums vectorised
    mean, _ = native.segment_reduce_csr(view, csr.rowptr, csr.perm, n, "mean")
    src = wide[:, 1:65].contiguous()
    deg = R.degrees(index, n).double()[:, None]
    r_mean = torch.zeros(n, 64, dtype=torch.float64).index_add_(0, index, src.double()) / deg.clamp(min=1)
    bound = (deg - 1).clamp(min=0) * U * R.ref_abs_sum(src, index, n) / deg.clamp(min=1) + U * r_mean.abs()
    _within((mean.cpu().double() - r_mean).abs(), bound, f"scalar walker N={n} mean")
    assert not bool(mean.cpu()[deg[:, 0] == 0].any())


def test_segment_softmax_scalar_walker_third_trip_on_an_offset_view(native):
    """Forward (one wave per destination) and backward (one wave per ROW: 4 N rows) of the scalar kernels."""
    n, index = _scalar_walker_case()
    wide = S.values(index.numel(), 72, seed=23)
    scores = S.scores_for(index.numel(), 3, seed=23)
    grad = S.values(n, 64, seed=24)
    view = wide.to(DEV)[:, 1:65]
    assert view.stride(0) == 72 and view.data_ptr() % 16 == 4
    csr = _csr(index, n)
    out, saved = native.segment_softmax_csr(view, scores.to(DEV), csr.rowptr, csr.perm, n)
    b = G.attention_bars(wide[:, 1:65].contiguous(), scores, index, n, grad)
    r_out, _, r_m, r_z = b["ref"]
    _within((out.cpu().double() - r_out).abs(), b["forward"], f"scalar walker N={n} forward")
    assert torch.equal(saved[:, 0].cpu().double(), r_m)
    _within((saved[:, 1].cpu().double() - r_z).abs(), b["saved_z"], f"scalar walker N={n} Z")
    assert index.numel() > 2 * 64 * _cus()
    g_src, g_s = native.segment_softmax_backward(grad.to(DEV), view, scores.to(DEV), out, saved, csr.col32)
    _within((g_src.cpu().double() - b["want_src"]).abs(), b["grad_src"], f"scalar walker {index.numel()} rows grad_src")
    _within((g_s.cpu().double() - b["want_score"]).abs(), b["grad_score"], f"scalar walker {index.numel()} rows grad_score")


# ------------------------------------------------------------------------------------------ for_chunk_destinations
def _chunk_case(trips, seed):
    """N destinations for `trips` trips of the chunk walker's 64 x CUs waves (64 destinations a trip each): five waves reach the
    last trip, and one more chunk holds ONE destination, which owns rows; E = N + N / 2."""
    cus = _cus()
    first_pass = 4096 * cus
    n = (trips - 1) * first_pass + 64 * 5 + 1
    assert n > 64 * cus and (trips - 1) * first_pass < n <= trips * first_pass and n % 64 == 1
    index = G.random_index(n, n + n // 2, seed=seed)
    return n, index


_CHUNK_SUMS = {}


@pytest.mark.parametrize("use_perm", [True, False], ids=["perm", "sorted"])  # (the upper decorator varies fastest)
@pytest.mark.parametrize("d,trips", [(4, 3), (12, 3), (64, 2)])
def test_scatter_sum_chunk_walker_later_trips_are_exact_on_integers(native, d, trips, use_perm):
    if (d, trips) not in _CHUNK_SUMS:  # built once for both row orders; only the latest case is kept
        _CHUNK_SUMS.clear()
        n, index = _chunk_case(trips, seed=d)
        small = _ints8(index.numel(), d, seed=100 + d)
        _CHUNK_SUMS[d, trips] = (n, index, small, torch.zeros(n, d, dtype=torch.int32).index_add_(0, index, small.int()))
    n, index, small, want = _CHUNK_SUMS[d, trips]  # want: integer arithmetic, exact
    assert int(want.abs().max()) < 2 ** 24 and bool(want[n - 1].any())
    src = small.to(DEV).float()
    rowptr, perm, _ = native.csr_build(index.to(DEV), n)
    if use_perm:
        out = native.scatter_sum_csr(src, rowptr, perm, n)
    else:  # messages already in destination-sorted order
        out = native.scatter_sum_csr(src[perm.long()], rowptr, None, n)
    assert torch.equal(out, want.to(DEV).float())


def test_segment_max_chunk_walker_third_trip(native):
    n, index = _chunk_case(3, seed=31)
    src = R.values(index.numel(), 4, seed=32)
    r_max, r_arg = G.max_first_row_wins(src, index, n)
    rowptr, perm, _ = native.csr_build(index.to(DEV), n)
    mx, arg = native.segment_reduce_csr(src.to(DEV), rowptr, perm, n, "max", with_argmax=True)
    assert _bits(mx, r_max.to(DEV)) and torch.equal(arg, r_arg.int().to(DEV))
    assert bool((r_arg[n - 1] >= 0).all()) and bool((r_arg == -1).any())
    # the mean through the same walker: the bound of tests/test_gpu_segment_reduce.py, its sums vectorised
    mean, _ = native.segment_reduce_csr(src.to(DEV), rowptr, perm, n, "mean")
    deg = R.degrees(index, n).double()[:, None]
    r_mean = torch.zeros(n, 4, dtype=torch.float64).index_add_(0, index, src.double()) / deg.clamp(min=1)
    bound = (deg - 1).clamp(min=0) * U * R.ref_abs_sum(src, index, n) / deg.clamp(min=1) + U * r_mean.abs()
    _within((mean.cpu().double() - r_mean).abs(), bound, f"chunk walker N={n} mean")


def test_segment_softmax_chunk_walker_third_trip(native):
    n, index = _chunk_case(3, seed=33)
    src, scores = S.values(index.numel(), 4, seed=34), S.scores_for(index.numel(), 3, seed=34)
    rowptr, perm, _ = native.csr_build(index.to(DEV), n)
    out, saved = native.segment_softmax_csr(src.to(DEV), scores.to(DEV), rowptr, perm, n)
    b = G.attention_bars(src, scores, index, n)
    r_out, _, r_m, r_z = b["ref"]
    _within((out.cpu().double() - r_out).abs(), b["forward"], f"chunk walker N={n} forward")
    assert torch.equal(saved[:, 0].cpu().double(), r_m)
    _within((saved[:, 1].cpu().double() - r_z).abs(), b["saved_z"], f"chunk walker N={n} Z")
    assert float(saved[n - 1, 1]) >= 1.0
