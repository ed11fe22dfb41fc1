"""GPU: ``functional.knn_graph`` / ``native.knn_graph_padded`` (csrc/knn_graph.hip, DESIGN K24) against the brute-force NumPy
reference of tests/knn_reference.py.  Every comparison is exact: integer equality for the edges, bit equality for ``dist``;
every call is also compared with a second run of itself.

Sizes follow what can go wrong in the kernel, read from ``native.knn_graph_constants()``: QUERY_BLOCK (64: the query rows of a
workgroup, one per lane - one below, at and one past it, and one past two blocks) and CANDIDATE_UNROLL (4: the unroll of the
candidate loop; its remainder path is taken at every count that is no multiple of it).  The kernel
stages nothing in LDS, so there is no candidate tile size; 4,100 nodes are 65 query blocks over 1,025 unrolled groups."""
import numpy as np
import pytest
import torch

from graphnet_classifier_amd import functional as F
from graphnet_classifier_amd import native
from tests import knn_reference as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(dist):
    return dist.view(torch.int32).cpu().numpy().view(np.uint32)


def _check(feat_np, k, graph_ptr=None, loop=False, feat_dev=None, device_ptr=False):
    """One call with dist and one without, a repeat, and the reference: all the same bits.  Returns the edges (NumPy)."""
    feat = _dev(feat_np) if feat_dev is None else feat_dev
    gp = graph_ptr
    if device_ptr:
        gp = torch.tensor(graph_ptr, dtype=torch.int64, device="cuda")
    ei, dist = F.knn_graph(feat, k, graph_ptr=gp, loop=loop, return_dist=True)
    only = F.knn_graph(feat, k, graph_ptr=gp, loop=loop)
    ei2, dist2 = F.knn_graph(feat, k, graph_ptr=gp, loop=loop, return_dist=True)
    N = feat_np.shape[0]
    assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, k * N) and dist.dtype == torch.float32 and tuple(dist.shape) == (k * N,)
    assert torch.equal(ei, only) and torch.equal(ei, ei2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32))
    want_ei, want_bits = R.knn_graph(feat_np, k, graph_ptr, loop)
    got = ei.cpu().numpy()
    assert np.array_equal(got, want_ei)
    assert np.array_equal(_bits(dist), want_bits)
    return got


@pytest.fixture(scope="module")
def constants():
    q, unroll = native.knn_graph_constants()
    assert q == 64 and unroll == 4  # the sizes below are chosen around these
    return q, unroll


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("k", [1, 3, 8])
def test_ties_on_the_integer_grid(k):
    grid = R.integer_grid(9)
    assert R.rows_cut_inside_a_tie(grid, k) >= 1  # not vacuous: the index half of the key decides some edge
    _check(grid, k)


@pytest.mark.parametrize("loop", [False, True])
def test_ties_between_duplicated_rows(loop):
    rng = np.random.default_rng(2)
    base = rng.standard_normal((10, 5)).astype(np.float32)
    feat = base[rng.integers(0, 10, 70)]  # 70 rows, 10 distinct: distance 0 between distinct nodes
    assert R.rows_cut_inside_a_tie(feat, 4, loop) >= 1
    got = _check(feat, 4, loop=loop)
    if loop:  # distance 0 to itself and to its copies: the smallest id of its copies comes first
        first = got[0].reshape(70, 4)[:, 0]
        assert all(np.array_equal(feat[first[v]], feat[v]) and first[v] <= v for v in range(70))
    else:
        assert (got[0] != got[1]).all()


# ------------------------------------------------------------------------------------------------ boundaries
@pytest.mark.parametrize("n", [9, 63, 64, 65, 66, 67, 127, 128, 129])
def test_sizes_around_the_query_block_and_the_unroll(constants, n):
    q, unroll = constants
    assert n == 9 or any(abs(n - m * q) <= 3 for m in (1, 2))
    rng = np.random.default_rng(n)
    _check(rng.standard_normal((n, 5)).astype(np.float32), 8)  # n = 9: k + 1 nodes, exactly enough candidates


def test_exactly_enough_candidates_at_the_largest_k():
    rng = np.random.default_rng(17)
    got = _check(rng.standard_normal((17, 3)).astype(np.float32), 16)
    assert (got >= 0).all()
    got = _check(rng.standard_normal((16, 3)).astype(np.float32), 16, loop=True)
    assert (got >= 0).all()


def test_one_large_graph():
    rng = np.random.default_rng(4100)
    _check(rng.standard_normal((4100, 5)).astype(np.float32), 16)


# ------------------------------------------------------------------------------------------------ parameters
@pytest.mark.parametrize("dim", [1, 5, 16])
@pytest.mark.parametrize("k", [1, 8, 16])
def test_dims_ks_and_a_strided_table(dim, k):
    rng = np.random.default_rng(100 * dim + k)
    wide = rng.standard_normal((150, dim + 3)).astype(np.float32)
    wide_dev = _dev(wide)
    view = wide_dev[:, 2:2 + dim]  # ld_feat = dim + 3 > dim, and a column offset: read where it lies
    assert view.stride(0) == dim + 3 and view.storage_offset() == 2
    _check(wide[:, 2:2 + dim], k, feat_dev=view)
    _check(np.ascontiguousarray(wide[:, 2:2 + dim]), k)


def test_dim_one_is_full_of_ties():
    feat = (np.arange(97) % 7).astype(np.float32).reshape(-1, 1)
    assert R.rows_cut_inside_a_tie(feat, 8) >= 1
    _check(feat, 8)


# ------------------------------------------------------------------------------------------------ batches
PTR = [0, 5, 70, 200, 209]  # ragged graphs of 5, 65, 130 and 9 nodes


@pytest.mark.parametrize("device_ptr", [False, True])
def test_ragged_batch_equals_each_graph_alone(device_ptr):
    rng = np.random.default_rng(7)
    feat = rng.standard_normal((209, 5)).astype(np.float32)
    got = _check(feat, 4, graph_ptr=PTR, device_ptr=device_ptr)
    for a, b in zip(PTR[:-1], PTR[1:]):
        alone = F.knn_graph(_dev(feat[a:b]), 4).cpu().numpy()
        part = got[:, 4 * a:4 * b]
        assert np.array_equal(part, alone + a)
        assert part.min() >= a and part.max() < b  # no edge crosses graphs
    assert np.array_equal(got[1], np.repeat(np.arange(209), 4))


def test_empty_graphs_inside_a_batch():
    rng = np.random.default_rng(8)
    feat = rng.standard_normal((140, 4)).astype(np.float32)
    _check(feat, 4, graph_ptr=[0, 0, 70, 70, 140, 140])


# ------------------------------------------------------------------------------------------------ padded entry
def test_padded_entry_equals_the_graph_ptr_entry():
    B, cap, k, counts_np = 3, 96, 8, [96, 40, 9]
    rng = np.random.default_rng(9)
    feat = rng.standard_normal((B, cap, 5)).astype(np.float32)
    for b, n in enumerate(counts_np):
        feat[b, n:] = 0.0  # garbage behind the count: all equal to each other and closer to the origin than most rows
    feat[1, 40:] = feat[1, 0]  # ... and copies of a live row: they would win every tie if they were read
    counts = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    counts[:, 0] = torch.tensor(counts_np, dtype=torch.int32)
    fd = _dev(feat)
    ei, dist, status = native.knn_graph_padded(fd, counts, k, return_dist=True)
    ei2, dist2, _ = native.knn_graph_padded(fd, counts, k, return_dist=True)
    assert tuple(ei.shape) == (B, 2, k * cap) and tuple(dist.shape) == (B, k * cap)
    assert torch.equal(ei, ei2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32))
    assert int(status.item()) == 0
    flat, _, _ = native.knn_graph_padded(fd, counts[:, 0].contiguous(), k)  # counts [B]: stride 1
    assert torch.equal(flat, ei)
    for b, n in enumerate(counts_np):
        want, want_dist = F.knn_graph(fd[b, :n], k, return_dist=True)
        ref_ei, ref_bits = R.knn_graph(feat[b, :n], k)
        assert np.array_equal(want.cpu().numpy(), ref_ei)
        assert torch.equal(ei[b, :, :k * n], want)  # local ids
        assert torch.equal(dist[b, :k * n].view(torch.int32), want_dist.view(torch.int32))
        assert np.array_equal(_bits(dist[b, :k * n]), ref_bits)
        assert bool((ei[b, :, k * n:] == -1).all())
        assert bool(torch.isinf(dist[b, k * n:]).all())
        assert int(ei[b, :, :k * n].max()) < n  # rows behind n_b never appear as neighbours


# ------------------------------------------------------------------------------------------------ flags
def test_too_few_candidates_on_a_device_graph_ptr():
    rng = np.random.default_rng(10)
    feat = rng.standard_normal((73, 5)).astype(np.float32)
    ptr = [0, 3, 73]
    gp = torch.tensor(ptr, dtype=torch.int64, device="cuda")
    ei, dist, status = F.knn_graph(_dev(feat), 8, graph_ptr=gp, return_dist=True, return_status=True)
    assert int(status.item()) == native.KNN_FEW_CANDIDATES
    want_ei, want_bits = R.knn_graph(feat, 8, ptr)
    got = ei.cpu().numpy()
    assert np.array_equal(got, want_ei) and np.array_equal(_bits(dist), want_bits)
    small = got[:, :24].reshape(2, 3, 8)
    assert (small[:, :, 2:] == -1).all() and (small[:, :, :2] >= 0).all() and (small[:, :, :2] < 3).all()
    assert got.min() >= -1 and got.max() < 73
    with pytest.raises(ValueError, match="graph 0 has 3 nodes"):
        F.knn_graph(_dev(feat), 8, graph_ptr=ptr)
    ok = F.knn_graph(_dev(feat), 2, graph_ptr=gp, return_status=True)
    assert int(ok[1].item()) == 0


def test_nan_feature_sets_the_nan_flag():
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((70, 5)).astype(np.float32)
    feat[33, 2] = np.nan
    fd = _dev(feat)
    ei, dist, status = F.knn_graph(fd, 8, return_dist=True, return_status=True)
    assert int(status.item()) == native.KNN_NAN_DISTANCE
    want_ei, want_bits = R.knn_graph(feat, 8)
    assert np.array_equal(ei.cpu().numpy(), want_ei) and np.array_equal(_bits(dist), want_bits)
    got = ei.cpu().numpy()[0].reshape(70, 8)
    assert not (np.delete(got, 33, axis=0) == 33).any()  # the NaN node is everybody's last choice
    assert (want_bits.reshape(70, 8)[33] == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------ topology
def test_topology_build_takes_the_list_whole():
    from graphnet_classifier_amd.GNN import scatter_mean
    from graphnet_classifier_amd.topology import GraphTopology, check_deferred
    rng = np.random.default_rng(12)
    feat = rng.standard_normal((209, 5)).astype(np.float32)
    k, N = 4, 209
    ei = F.knn_graph(_dev(feat), k, graph_ptr=PTR)
    E = k * N
    *_, flags = native.topology_build(ei[0].contiguous(), ei[1].contiguous(), N, gated_fallback=True)
    assert flags.tolist() == [0, 0, 0]  # in range, and the gated general path was never raised
    for validate in (True, "deferred"):
        topo = GraphTopology(ei, N, validate=validate)
        assert torch.equal(topo.perm.to(torch.int64), torch.arange(E, device="cuda"))
        assert torch.equal(topo.rowptr.to(torch.int64), k * torch.arange(N + 1, device="cuda"))
    check_deferred()
    x = torch.from_numpy(rng.standard_normal((N, 8)).astype(np.float32)).cuda()
    src = x[ei[0]]  # the senders' rows, one per edge
    mean = scatter_mean(src, ei[1], dim_size=N)
    rows = src.view(N, k, 8)
    want = (((rows[:, 0] + rows[:, 1]) + rows[:, 2]) + rows[:, 3]) / 4.0  # the kernel's order: from +0.0, ascending slots
    assert torch.equal(mean, want)


# ------------------------------------------------------------------------------------------------ capture
def test_capture_and_replay_with_new_features():
    rng = np.random.default_rng(13)
    a = rng.standard_normal((209, 5)).astype(np.float32)
    b = rng.standard_normal((209, 5)).astype(np.float32)
    gp = torch.tensor(PTR, dtype=torch.int64, device="cuda")
    buf = _dev(a)
    F.knn_graph(buf, 4, graph_ptr=gp)  # warm-up: library and allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ei, dist, status = F.knn_graph(buf, 4, graph_ptr=gp, return_dist=True, return_status=True)
    for feat in (a, b, a):
        buf.copy_(_dev(feat))
        graph.replay()
        torch.cuda.synchronize()
        want, want_dist = F.knn_graph(_dev(feat), 4, graph_ptr=gp, return_dist=True)
        assert torch.equal(ei, want) and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32))
        assert np.array_equal(ei.cpu().numpy(), R.knn_graph(feat, 4, PTR)[0])
        assert int(status.item()) == 0
