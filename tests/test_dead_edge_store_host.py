"""Host side of the aggregate-only edge launch (no GPU): the shape query gnc_mlp_agg_only_supported and the model's choice of
which block may drop its edge output."""
import ctypes
import types

import pytest
import torch

FAKE = 0x10000  # never dereferenced by the shape queries; 16-B aligned


def _edge_desc(native, rows=10_000_000, width=64, num_linear=3, ln=True):
    """The W-split edge processor's description at c3 as the binding lists it for the kernel: the MATMUL segment (also the
    residual) first, then the two gathered ADD segments."""
    d = native.MlpDesc()
    d.num_segments, d.num_linear, d.activation = 3, num_linear, 0
    for s in (1, 2):
        g = d.seg[s]
        g.ptr, g.index, g.width, g.ld, g.mode, g.table_rows = FAKE, FAKE, width, width, native.SEG_ADD, 1_000_000
    m = d.seg[0]
    m.ptr, m.width, m.ld, m.mode, m.wcol = FAKE + 0x100000, width, width, native.SEG_MATMUL, 0
    for l in range(num_linear):
        d.in_dim[l], d.out_dim[l], d.weight[l] = width, width, FAKE
    if ln:
        d.ln_gamma, d.ln_beta, d.ln_eps = FAKE, FAKE, 1e-5
    d.residual, d.ld_residual = FAKE + 0x100000, width
    d.out, d.ld_out, d.rows = FAKE, width, rows
    d.agg_out, d.ld_agg, d.agg_index, d.agg_fix = FAKE, width, FAKE, FAKE
    return d


def test_agg_only_query_serves_the_c3_edge_processor_only():
    from graphnet_classifier_amd import native
    lib = native.load_library()
    q = lambda d: lib.gnc_mlp_agg_only_supported(ctypes.byref(d))  # noqa: E731
    d = _edge_desc(native)
    assert lib.gnc_mlp_agg_supported(ctypes.byref(d)) == 0 and q(d) == 0
    assert q(_edge_desc(native, rows=40_003)) == 0                      # fewer tiles than waves: still served
    assert q(_edge_desc(native, rows=1_000)) == 0                       # 64 wide: no small-batch kernel in front
    d = _edge_desc(native, width=48)                                    # not every width 64: the storing launch
    assert lib.gnc_mlp_agg_supported(ctypes.byref(d)) == 0 and q(d) != 0
    assert b"agg_only_supported" in lib.gnc_last_error_string()
    assert q(_edge_desc(native, num_linear=2)) != 0
    assert q(_edge_desc(native, ln=False)) != 0
    d = _edge_desc(native)
    d.save_act[0], d.save_act[1] = FAKE, FAKE                           # training forward keeps storing
    assert q(d) != 0
    d = _edge_desc(native)
    d.residual = FAKE + 0x200000                                        # residual not the staged rows
    assert q(d) != 0


def test_graph_processor_lets_only_the_last_block_drop_its_edges():
    from graphnet_classifier_amd import GNN as G
    gp = G.GraphProcessor(3, 8, 8, 8, 8)
    seen = []
    for k, b in enumerate(gp.blocks):
        def fwd(x, topo, e, need_edges=True, k=k):
            seen.append((k, need_edges))
            return x, (None if not need_edges else e)
        b.forward_sorted = fwd
    x, e = torch.zeros(2, 8), torch.zeros(3, 8)
    gp.forward_sorted(x, None, e)
    assert seen == [(0, True), (1, True), (2, True)]
    seen.clear()
    _, eo = gp.forward_sorted(x, None, e, need_edges=False)
    assert seen == [(0, True), (1, True), (2, False)] and eo is None


@pytest.mark.parametrize("grad", [False, True])
def test_edge_processor_asks_for_the_aggregate_only_launch_in_inference_only(grad, monkeypatch):
    from graphnet_classifier_amd import GNN as G
    from graphnet_classifier_amd import functional as Fn
    ep = G.EdgeProcessor(8, 8, 8)
    got = {}
    monkeypatch.setattr(Fn, "edge_processor_wsplit_aggregated", lambda *a, **k: got.update(inf=k) or (None, "agg"))
    monkeypatch.setattr(Fn, "edge_processor_wsplit", lambda *a, **k: got.update(train=k) or ("e", "agg"))
    topo = types.SimpleNamespace(num_edges=3)
    x, e = torch.zeros(2, 8), torch.zeros(3, 8)
    with torch.set_grad_enabled(grad):
        ep.forward_sorted(x, topo, e, aggregate=True, need_edges=False)
    if grad:
        assert "train" in got and "inf" not in got
    else:
        assert got["inf"].get("store_edges") is False
    got.clear()
    with torch.no_grad():
        ep.forward_sorted(x, topo, e, aggregate=True)
    assert got["inf"].get("store_edges") is True
