"""GPU: the top-K node pooling kernels (K20, csrc/topk_pool.hip) at operator level against the integer / float64 reference of
tests/topk_pool_cases.py.  Integer outputs (new ids, kept rows, offsets, the filtered edge list, its CSR offsets) are compared for
EQUALITY; gated rows and gradients against float64 under the project's bar, 1e-5 max(1, |reference|), into NaN-prefilled outputs."""
import numpy as np
import pytest
import torch

from tests import topk_pool_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _select(scores, graph_ptr, ratio):
    """Device select, narrowed by ONE read-back; compared with the reference; returns the device tensors and N'."""
    from graphnet_classifier_amd import native
    new_id, kept, gp_out, counts = native.topk_pool_select(_dev(scores), _dev(np.asarray(graph_ptr, np.int64)), ratio)
    n_out = int(counts[0].item())
    ref_id, ref_kept, ref_gp = K.ref_select(scores, graph_ptr, ratio)
    assert n_out == ref_kept.size == int(ref_gp[-1])
    assert np.array_equal(new_id.cpu().numpy(), ref_id)
    assert np.array_equal(kept[:n_out].cpu().numpy(), ref_kept)
    assert np.array_equal(gp_out.cpu().numpy(), ref_gp)
    return new_id, kept, gp_out, counts, n_out


def _batch_ptr(sizes, front=0):
    return np.concatenate([[front], front + np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("ratio", K.RATIOS)
def test_select_every_size_in_one_batch(ratio):
    """The fifteen sizes as the graphs of one batch (an empty graph among them), 5 rows in front of graph_ptr[0] and 9 behind
    graph_ptr[G], every score pattern."""
    rng = np.random.default_rng(7)
    gp = _batch_ptr(K.SIZES, front=5)
    rows = int(gp[-1]) + 9
    for name, scores in K.score_patterns(rng, rows).items():
        _, _, _, _, n_out = _select(scores, gp, ratio)
        if ratio == 1.0:
            assert n_out == sum(K.SIZES), name


@pytest.mark.parametrize("graphs", (1, 3, 64, 300))
def test_select_batches(graphs):
    rng = np.random.default_rng(graphs)
    sizes = rng.integers(90, 210, size=graphs)
    if graphs >= 3:
        sizes[graphs // 2] = 0  # an empty graph in the middle
    gp = _batch_ptr(sizes, front=3)
    rows = int(gp[-1]) + 4
    for name, scores in K.score_patterns(rng, rows).items():
        for ratio in (0.5, 1e-3):
            _select(scores, gp, ratio)


def test_select_ceil_pairs_and_offsets_outside_the_table():
    rng = np.random.default_rng(3)
    for ratio, n in K.CEIL_PAIRS:
        _, _, _, _, n_out = _select(rng.standard_normal(n).astype(np.float32), [0, n], ratio)
        assert n_out == K.keep_count(ratio, n)
    _select(rng.standard_normal(300).astype(np.float32), [-4, 10, 10, 290, 350], 0.5)  # clamped as K17's graph_range
    _select(np.zeros(0, np.float32), [0, 0], 0.5)                                       # no rows at all


def test_select_is_a_function_of_the_graph_alone():
    """The same bits twice, and the same kept set for a graph alone or at any position of a batch."""
    from graphnet_classifier_amd import native
    rng = np.random.default_rng(11)
    sizes = (257, 64, 1025, 3)
    parts = [K.score_patterns(rng, n)["duplicates"] for n in sizes]
    gp = _batch_ptr(sizes, front=2)
    scores = np.concatenate([np.zeros(2, np.float32)] + parts + [np.zeros(6, np.float32)])
    a = native.topk_pool_select(_dev(scores), _dev(gp), 0.25)
    b = native.topk_pool_select(_dev(scores), _dev(gp), 0.25)
    n_out = int(a[3][0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][:n_out], b[1][:n_out]) and torch.equal(a[2], b[2]) and int(b[3][0]) == n_out
    inside = a[0].cpu().numpy()
    for g, part in enumerate(parts):
        alone, _, _, _, _ = _select(part, [0, part.size], 0.25)
        lo, hi = int(gp[g]), int(gp[g + 1])
        assert np.array_equal(inside[lo:hi] >= 0, alone.cpu().numpy() >= 0), g


def _filter(src, dst, rowptr, new_id_dev, kept_dev, counts, ref_id):
    from graphnet_classifier_amd import native
    E = src.size
    out = native.topk_pool_filter_edges(_dev(src), _dev(dst), _dev(rowptr), new_id_dev, kept_dev, counts)
    n_out, e_out = counts.tolist()
    s_ref, d_ref, ke_ref, eid_ref, rp_ref = K.ref_filter(src, dst, rowptr, ref_id)
    s, d, ke, eid, rp = (t.cpu().numpy() for t in out)
    assert e_out == ke_ref.size and n_out == int((ref_id >= 0).sum())
    assert np.array_equal(s[:e_out], s_ref) and np.array_equal(d[:e_out], d_ref) and np.array_equal(ke[:e_out], ke_ref)
    assert np.array_equal(eid, eid_ref) and eid.size == E
    assert np.array_equal(rp[:n_out + 1], rp_ref)
    # what the reference implies, stated on the device result itself
    assert np.all(np.diff(d[:e_out]) >= 0) and np.all(np.diff(ke[:e_out]) > 0)
    assert np.array_equal(rp[:n_out + 1], np.concatenate([[0], np.cumsum(np.bincount(d[:e_out], minlength=n_out))]))
    return e_out


@pytest.mark.parametrize("E", K.EDGE_COUNTS)
def test_filter_edges_at_every_edge_count(E):
    rng = np.random.default_rng(E + 1)
    rows = 700
    scores = rng.standard_normal(rows).astype(np.float32)
    gp = [0, 300, 300, 700]
    for ratio in (0.5, 1.0):
        new_id, kept, _, counts, _ = _select(scores, gp, ratio)
        src, dst, rowptr = K.sorted_edges(rng, rows, E, hub=True)
        e_out = _filter(src, dst, rowptr, new_id, kept, counts, K.ref_select(scores, gp, ratio)[0])
        if ratio == 1.0:
            assert e_out == E  # the inputs' bits back (asserted element by element against the reference above)


def test_filter_edges_patterns():
    rng = np.random.default_rng(5)
    rows = 520
    scores = rng.standard_normal(rows).astype(np.float32)
    gp = [10, 500]  # rows in front of and behind the graph are dropped, and so is every edge that touches them
    new_id, kept, _, counts, _ = _select(scores, gp, 0.5)
    ref_id = K.ref_select(scores, gp, 0.5)[0]
    src, dst, rowptr = K.sorted_edges(rng, rows, 3000, hub=True, out_of_range=6)  # endpoints outside [0, rows), both sides
    assert rowptr[0] == 2 and rowptr[-1] == src.size - 2
    assert _filter(src, dst, rowptr, new_id, kept, counts, ref_id) > 0
    # all edges dropped: every source is an erased node
    erased = np.nonzero(ref_id < 0)[0].astype(np.int32)
    src2 = erased[rng.integers(0, erased.size, size=src.size)]
    assert _filter(src2, dst, rowptr, new_id, kept, counts, ref_id) == 0
    # self-loops only: exactly the kept nodes' loops survive
    loops = np.arange(rows, dtype=np.int32)
    assert _filter(loops, loops, np.arange(rows + 1, dtype=np.int32), new_id, kept, counts, ref_id) == int((ref_id >= 0).sum())


def _bar(got, ref):
    """Worst |got - ref| / max(1, |ref|) in units of the bar 1e-5."""
    ref = ref.double()
    return float(((got.double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max()) / 1e-5 if ref.numel() else 0.0


@pytest.mark.parametrize("C", K.WIDTHS)
@pytest.mark.parametrize("padded", (False, True))
def test_rows_forward_and_backward(C, padded):
    """Gated and ungated compaction, into NaN-prefilled outputs, with and without a leading dimension above C."""
    from graphnet_classifier_amd import native
    rng = np.random.default_rng(C)
    rows, gp = 1031, [3, 400, 400, 1029]
    scores = (2.0 * rng.standard_normal(rows)).astype(np.float32)
    new_id, kept, _, _, n_out = _select(scores, gp, 0.5)
    kept = kept[:n_out]
    ld = C + (4 if C % 4 == 0 else 3) if padded else C
    x_full = torch.from_numpy(rng.standard_normal((rows, ld)).astype(np.float32)).to(DEV)
    g_full = torch.from_numpy(rng.standard_normal((n_out, ld)).astype(np.float32)).to(DEV)
    x, grad = x_full[:, :C], g_full[:, :C]
    s = _dev(scores)
    worst = 0.0
    for gated in (True, False):
        ref_out, ref_dx, ref_ds = K.ref_rows(x.cpu(), scores if gated else None, kept.cpu().numpy(), grad.cpu())
        out_full = torch.full((n_out, ld), float("nan"), device=DEV)
        out = native.topk_pool_rows_forward(x, kept, s if gated else None, out=out_full[:, :C])
        assert not bool(torch.isnan(out).any()) and (not padded or bool(torch.isnan(out_full[:, C:]).all()))
        if gated:
            worst = max(worst, _bar(out, ref_out))
        else:
            assert torch.equal(out, x[kept.long()])  # no gate: the bits of x
        dx_full = torch.full((rows, ld), float("nan"), device=DEV)
        ds_buf = torch.full((rows,), float("nan"), device=DEV)
        dx, ds = native.topk_pool_rows_backward(grad, new_id, x if gated else None, s if gated else None, dx=dx_full[:, :C],
                                                ds=ds_buf if gated else None)
        assert not bool(torch.isnan(dx).any()) and (not padded or bool(torch.isnan(dx_full[:, C:]).all()))
        dropped = new_id < 0
        assert bool(dropped.any()) and not bool(dx[dropped].ne(0).any()) and not bool(torch.signbit(dx[dropped]).any())  # exact +0.0
        worst = max(worst, _bar(dx, ref_dx))
        if gated:
            assert not bool(torch.isnan(ds).any()) and not bool(ds[dropped].ne(0).any()) and not bool(torch.signbit(ds[dropped]).any())
            worst = max(worst, _bar(ds, ref_ds))
            only_ds = native.topk_pool_rows_backward(grad, new_id, x, s, need_dx=False)
            only_dx = native.topk_pool_rows_backward(grad, new_id, x, s, need_ds=False)
            assert only_ds[0] is None and torch.equal(only_ds[1], ds) and only_dx[1] is None and torch.equal(only_dx[0], dx)
        else:
            assert ds is None and torch.equal(dx[~dropped], grad[new_id[~dropped].long()])
    print(f"C = {C}, ld = {ld}: worst error {worst:.3f} bars")
    assert worst <= 1.0


@pytest.mark.parametrize("C", (1, 64))
def test_row_launches_beyond_two_passes_of_the_capped_grid(C):
    """The three capped launches - rows_forward over the N' kept rows and rows_backward over all rows (8 workgroups per CU,
    256 / lanes rows each per trip) and, at C = 1, the CSR-offset kernel of the edge filter (8 x 256 rows per CU) - at two full
    passes and 1027 rows more for the SMALLEST of them (N' at ratio 0.5): graphs of up to 4,097 rows, checked as everywhere here."""
    from graphnet_classifier_amd import native
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lanes = {1: 1, 64: 16}[C]
    first_pass = 8 * cus * (256 // lanes)
    rows = 2 * (2 * first_pass + 1027)
    rng = np.random.default_rng(17 + C)
    sizes = []
    while sum(sizes) < rows - 9:
        sizes.append(min(int(rng.integers(2000, 4098)), rows - 9 - sum(sizes)))
    gp = _batch_ptr(sizes, front=5)
    assert int(gp[-1]) == rows - 4
    scores = (2.0 * rng.standard_normal(rows)).astype(np.float32)
    new_id, kept, _, counts, n_out = _select(scores, gp, 0.5)
    assert n_out > 2 * first_pass and rows + 1 > 2 * first_pass and (C != 1 or rows + 1 > 2 * 8 * cus * 256)
    if C == 1:  # the edge filter's rowptr launch over rows + 1 entries
        src, dst, rowptr = K.sorted_edges(rng, rows, rows, hub=True)
        assert _filter(src, dst, rowptr, new_id, kept, counts, K.ref_select(scores, gp, 0.5)[0]) > 0
    kept = kept[:n_out]
    x =torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32)).to(DEV)
    grad = torch.from_numpy(rng.standard_normal((n_out, C)).astype(np.float32)).to(DEV)
    s = _dev(scores)
    ref_out, ref_dx, ref_ds = K.ref_rows(x.cpu(), scores, kept.cpu().numpy(), grad.cpu())
    out = native.topk_pool_rows_forward(x, kept, s, out=torch.full((n_out, C), float("nan"), device=DEV))
    dx, ds = native.topk_pool_rows_backward(grad, new_id, x, s, dx=torch.full((rows, C), float("nan"), device=DEV),
                                            ds=torch.full((rows,), float("nan"), device=DEV))
    dropped = new_id < 0
    assert bool(dropped.any()) and not bool(dx[dropped].ne(0).any()) and not bool(ds[dropped].ne(0).any())
    worst = max(_bar(out, ref_out), _bar(dx, ref_dx), _bar(ds, ref_ds))
    print(f"C = {C}, {rows} rows, {n_out} kept: worst error {worst:.3f} bars")
    assert worst <= 1.0
    plain = native.topk_pool_rows_forward(x, kept, None)
    assert torch.equal(plain, x[kept.long()])  # no gate: the bits of x
    dx_plain, _ = native.topk_pool_rows_backward(grad, new_id, None, None)
    assert torch.equal(dx_plain[~dropped], grad[new_id[~dropped].long()]) and not bool(dx_plain[dropped].ne(0).any())


def test_functional_topk_pool_on_a_grid_and_its_gradients():
    """``Fn.topk_pool`` end to end on the 128 x 128 grid's edges (16,384 nodes, 32,512 edges, ONE graph of the largest size): the
    pooled topology is the reference's and serves the aggregation kernels; autograd reaches x, the scores and the edge rows."""
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd.topology import GraphTopology
    from oracle import graphnet_oracle as O
    rng = np.random.default_rng(1)
    n, C, De = 128 * 128, 8, 4
    ei = torch.from_numpy(O.grid_edge_index(128, 128))
    topo = GraphTopology(ei.to(DEV), n, device=DEV)
    scores = rng.standard_normal(n).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).to(DEV).requires_grad_(True)
    e = torch.from_numpy(rng.standard_normal((ei.size(1), De)).astype(np.float32)).to(DEV).requires_grad_(True)
    s = _dev(scores).requires_grad_(True)
    gp = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    x2, e2, topo2, gp2, kept = Fn.topk_pool(x, s, topo, gp, 0.5, e)
    ref_id, ref_kept, ref_gp = K.ref_select(scores, [0, n], 0.5)
    src, dst, rowptr = (t.cpu().numpy() for t in (topo.src_sorted, topo.dst_sorted, topo.rowptr))
    s_ref, d_ref, ke_ref, _, rp_ref = K.ref_filter(src, dst, rowptr, ref_id)
    assert np.array_equal(kept.cpu().numpy(), ref_kept) and gp2.tolist() == ref_gp.tolist() == [0, n // 2]
    assert topo2.num_nodes == n // 2 and topo2.num_edges == ke_ref.size and topo2.status is topo.status and not topo2.deferred
    assert np.array_equal(topo2.src_sorted.cpu().numpy(), s_ref) and np.array_equal(topo2.dst_sorted.cpu().numpy(), d_ref)
    assert np.array_equal(topo2.rowptr.cpu().numpy(), rp_ref) and torch.equal(topo2.perm.long(), torch.arange(ke_ref.size, device=DEV))
    assert torch.equal(e2, e[torch.from_numpy(ke_ref.astype(np.int64)).to(DEV)])
    agg = Fn.scatter_sum_csr(e2.detach(), topo2.rowptr, None, topo2.dst_sorted, topo2.num_nodes)  # the pooled CSR under K1
    want = torch.zeros(n // 2, De, dtype=torch.float64).index_add_(0, torch.from_numpy(d_ref.astype(np.int64)), e2.detach().double().cpu())
    assert _bar(agg, want) <= 1.0
    rp_csc, _ = topo2.csc  # lazy, unchanged
    assert rp_csc.numel() == n // 2 + 1 and int(rp_csc[-1]) == ke_ref.size
    gx, ge = torch.randn_like(x2), torch.randn_like(e2)
    (x2 * gx).sum().add((e2 * ge).sum()).backward()
    _, ref_dx, ref_ds = K.ref_rows(x.detach().cpu(), scores, ref_kept, gx.cpu())
    assert _bar(x.grad, ref_dx) <= 1.0 and _bar(s.grad, ref_ds) <= 1.0
    de = torch.zeros_like(e)
    de[torch.from_numpy(ke_ref.astype(np.int64)).to(DEV)] = ge
    assert torch.equal(e.grad, de)
    # nodes only (behind the last block): no topology, the same rows
    x3, e3, topo3, gp3, kept3 = Fn.topk_pool(x.detach(), s.detach(), topo, gp, 0.5, None, need_edges=False)
    assert e3 is None and topo3 is None and torch.equal(x3, x2.detach()) and torch.equal(kept3, kept) and torch.equal(gp3, gp2)
