"""The aggregate-only edge launch (gnc_mlp_forward_agg_only_f32): the last GN block's edge processor in inference forms the
node model's aggregate without storing its e' rows.  The aggregate must be bit for bit the storing launch's, at c3-like sizes
and at the edges of the wave-range bookkeeping (partial last tile, empty destinations, a destination that spans many wave
ranges, a batch that leaves waves of the persistent grid idle), and the model's output must not change."""
import numpy as np
import pytest
import torch

DEV = "cuda"
pytestmark = pytest.mark.gpu


def _rowptr(dst, nodes):
    counts = torch.bincount(dst.long(), minlength=nodes)
    return torch.cat([torch.zeros(1, dtype=torch.long, device=dst.device), counts.cumsum(0)]).to(torch.int32)


def _edge_case(rows, nodes, seed, hub=None, empty=None):
    """W-split edge processor inputs at width 64; ``hub`` = (node, rows) gives one destination that many rows, ``empty`` a range
    of destinations without rows."""
    rng = np.random.default_rng(seed)
    dst = rng.integers(0, nodes, rows)
    if empty is not None:
        lo, hi = empty
        dst = np.where((dst >= lo) & (dst < hi), lo - 1, dst)
    if hub is not None:
        v, n = hub
        dst[:n] = v
    dst = np.sort(dst).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    ws, bs = [], []
    for _ in range(3):
        ws.append(t(rng.uniform(-0.125, 0.125, (64, 64)).astype(np.float32)))
        bs.append(t(rng.uniform(-0.125, 0.125, (64,)).astype(np.float32)))
    ln = (t(rng.uniform(0.5, 1.5, 64).astype(np.float32)), t(rng.uniform(-0.5, 0.5, 64).astype(np.float32)), 1e-5)
    c = dict(x=t(rng.standard_normal((rows, 64)).astype(np.float32)), ps=t(rng.standard_normal((nodes, 64)).astype(np.float32)),
             pd=t(rng.standard_normal((nodes, 64)).astype(np.float32)), src=t(rng.integers(0, nodes, rows).astype(np.int32)),
             dst=t(dst), ws=ws, bs=bs, ln=ln, nodes=nodes, rows=rows)
    c["rowptr"] = _rowptr(c["dst"], nodes)
    return c


def _launch(native, c, agg_only):
    segs = [(c["ps"], c["src"]), (c["pd"], c["dst"]), (c["x"], None)]
    return native.mlp_forward(segs, c["ws"], c["bs"], ln=c["ln"], residual=c["x"], rows=c["rows"],
                              modes=[native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL],
                              aggregate=(c["dst"], c["rowptr"], c["nodes"]), agg_only=agg_only)


CASES = {
    # c3-like: ~10 rows per destination, a row count that is not a multiple of 32, a band of empty destinations
    "c3_like": dict(rows=2_000_017, nodes=200_000, seed=1, empty=(1000, 1400)),
    # one destination spans many wave ranges (a range is ~150 rows here), others have no rows at all
    "hub": dict(rows=300_001, nodes=5_000, seed=2, hub=(2_500, 40_000), empty=(10, 500)),
    # above the small-batch limit but fewer tiles than waves in the persistent grid: idle waves
    "idle_waves": dict(rows=40_003, nodes=4_000, seed=3, empty=(100, 130)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_agg_only_launch_matches_the_storing_launch_bit_for_bit(name):
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import native
    lib = native.load_library()
    c = _edge_case(**CASES[name])
    out, agg = _launch(native, c, agg_only=False)
    none, agg_o = _launch(native, c, agg_only=True)
    torch.cuda.synchronize()
    assert agg is not None and out is not None
    assert none is None, "the aggregate-only launch did not serve this shape"
    assert lib.gnc_mlp_agg_only_supported is not None
    assert torch.equal(agg_o, agg)
    # and both are K1 on the stored rows
    assert torch.equal(agg, Fn.scatter_sum_csr(out, c["rowptr"], None, c["dst"], c["nodes"]))
    again = _launch(native, c, agg_only=True)[1]
    assert torch.equal(again, agg_o)


def _model(G, S, n_blocks, graphs=48, seed=7):
    batch = S.random_pair_graphs(graphs, 160, 800, 3, seed)  # c3's graphs: 1600 edges each, above the small-batch limit
    torch.manual_seed(seed)
    m = G.GraphNet(**S.graphnet_kwargs(64, n_blocks)).to(DEV)
    return m, batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)


@pytest.mark.parametrize("n_blocks", [1, 2, 3])
def test_graphnet_forward_unchanged_and_last_block_stores_nothing(n_blocks, monkeypatch):
    from graphnet_classifier_amd import GNN as G
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import synthetic as S
    m, x, pos, ei = _model(G, S, n_blocks)
    calls = []
    real = Fn.edge_processor_wsplit_aggregated

    def spy(*a, **k):
        r = real(*a, **k)
        calls.append((k.get("store_edges", True), r[0] is None))
        return r

    monkeypatch.setattr(Fn, "edge_processor_wsplit_aggregated", spy)
    outs = {}
    for drop in (False, True):
        monkeypatch.setattr(G, "DROP_DEAD_EDGE_STORE", drop)
        calls.clear()
        with torch.no_grad():
            outs[drop] = m(x, pos, ei)
        torch.cuda.synchronize()
        if drop:  # every block but the last stores e'; the last one does not
            assert calls == [(True, False)] * (n_blocks - 1) + [(False, True)]
        else:
            assert calls == [(True, False)] * n_blocks
    assert torch.equal(outs[True], outs[False])
    # with autograd on (training) every block stores e'
    calls.clear()
    y = m(x, pos, ei)
    assert all(not none for _, none in calls)
    assert float((y.detach() - outs[True]).abs().max()) < 1e-5


def test_block_and_processor_entry_points_keep_their_edge_output():
    from graphnet_classifier_amd import GNN as G
    from graphnet_classifier_amd import synthetic as S
    m, x, pos, ei = _model(G, S, 2, graphs=24)
    xn = torch.randn(x.size(0), 64, device=DEV)
    ea = torch.randn(ei.size(1), 64, device=DEV)
    with torch.no_grad():
        xo, eo = m.graph_processor(xn, ei, ea)
        xb, eb, _ = m.graph_processor.blocks[-1](xn, ei, ea)
    assert eo is not None and eo.shape == ea.shape and bool(torch.isfinite(eo).all())
    assert eb is not None and eb.shape == ea.shape and bool(torch.isfinite(eb).all())


def test_deferred_validation_still_poisons_with_the_aggregate_only_block():
    from graphnet_classifier_amd import GNN as G
    from graphnet_classifier_amd import synthetic as S
    from graphnet_classifier_amd import topology
    assert G.DROP_DEAD_EDGE_STORE
    m, x, pos, ei = _model(G, S, 1, graphs=24)
    bad = ei.clone()
    bad[0, 5] = x.size(0) + 3
    topology.set_validation("deferred")
    try:
        topology.clear_topology_cache()
        with torch.no_grad():
            good = m(x, pos, ei)
            poisoned = m(x, pos, bad)
        assert bool(torch.isfinite(good).all())
        assert bool(torch.isnan(poisoned).all())
        with pytest.raises(IndexError):
            topology.check_deferred()
    finally:
        topology.set_validation("sync")
        topology.clear_topology_cache()
