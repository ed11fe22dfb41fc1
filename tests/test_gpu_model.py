"""GPU parity of the module surface (graphnet_classifier_amd.GNN / .MLP) against the golden
vectors captured from the reference and against the CPU oracle.  Tolerance: 1e-5 absolute
fp32 (BASELINE.json north_star), on outputs of O(0.1 .. 1).
"""
import ast

import numpy as np
import pytest
import torch

from oracle import graphnet_oracle as O
from tests._util import load_golden, max_abs, sub_state_dict, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


@pytest.fixture(scope="module")
def G():
    from graphnet_classifier_amd import GNN
    return GNN


def _kwargs(g):
    return ast.literal_eval(bytes(g["kwargs_json"]).decode())


def test_native_library_is_loaded(G):
    """The HIP extension must be the thing that runs: the in-tree .so is mapped into this process."""
    from graphnet_classifier_amd import native
    native.load_library()
    with open("/proc/self/maps") as f:
        assert "libgnc_hip.so" in f.read()


def test_scatter_sum_public_api(G):
    g = load_golden("g1_scatter.npz")
    src, index = t(g["src"]), t(g["index"])
    out = G.scatter_sum(src.to(DEV), index.to(DEV), dim=0)
    assert out.is_cuda and torch.equal(out.cpu(), t(g["out_infer"]))
    # CPU tensors in -> result comes back on the CPU (the reference's callers never place tensors)
    out_cpu = G.scatter_sum(src, index, dim=0, dim_size=40)
    assert not out_cpu.is_cuda and torch.equal(out_cpu, t(g["out_dimsize40"]))
    out1d = G.scatter_sum(t(g["src1d"]).to(DEV), index.to(DEV))
    assert out1d.shape == (37, 1) and torch.equal(out1d.cpu(), t(g["out_1d"]))
    assert tuple(G.scatter_sum(torch.zeros(0, 8, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV)).shape) == (0, 8)
    with pytest.raises(NotImplementedError):
        G.scatter_sum(src.to(DEV), index.to(DEV), dim=1)
    with pytest.raises(IndexError):
        G.scatter_sum(src.to(DEV), index.to(DEV), dim=0, dim_size=5)


def test_g3_processors_and_block(G):
    g = load_golden("g3_gnblock.npz")
    x, ei, ea = t(g["x"], DEV), t(g["edge_index"], DEV), t(g["edge_attr"], DEV)
    ep = G.EdgeProcessor(16, 8, hidden_dim=24, hidden_layers=2)
    ep.load_state_dict(sub_state_dict(g, "ep/sd/"))
    assert max_abs(ep(x[ei[0]], x[ei[1]], ea).cpu(), t(g["edge_out"])) < TOL
    npr = G.NodeProcessor(16, 8, hidden_dim=24, hidden_layers=2)
    npr.load_state_dict(sub_state_dict(g, "np/sd/"))
    assert max_abs(npr(x, ei, ea).cpu(), t(g["node_out"])) < TOL
    blk = G.build_GN_block(16, 8, hidden_dim_node=24, hidden_dim_edge=24)
    blk.load_state_dict(sub_state_dict(g, "blk/sd/"))
    bx, be, u = blk(x, ei, ea)
    assert u is None
    assert max_abs(bx.cpu(), t(g["block_x"])) < TOL and max_abs(be.cpu(), t(g["block_e"])) < TOL


def test_g4_graphnet_tiny(G):
    g = load_golden("g4_graphnet_tiny.npz")
    m = G.GraphNet(**_kwargs(g))
    m.load_state_dict(sub_state_dict(g, "sd/"), strict=True)
    with torch.no_grad():
        y = m(t(g["x"], DEV), t(g["pos"], DEV), t(g["edge_index"], DEV))
    assert y.shape == g["y"].shape and max_abs(y.cpu(), t(g["y"])) < TOL


def test_g4_graphnet_default_width_pixel_graph(G):
    g = load_golden("g4_graphnet_default.npz")
    m = G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3)  # main.py:72
    m.load_state_dict(sub_state_dict(g, "sd/"), strict=True)
    with torch.no_grad():
        y = m(t(g["x"]), t(g["pos"]), t(g["edge_index"]))  # host tensors, as the reference's loader yields
    assert not y.is_cuda and y.shape == (1024, 1)
    assert max_abs(y, t(g["y"])) < TOL


def test_g4_shipped_checkpoint_loads_strict_and_matches(G):
    g = load_golden("g4_graphnet_ckpt.npz")
    m = G.CombinedModel(G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=1024, classes=2)
    missing = m.load_state_dict(sub_state_dict(g, "sd/"), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.eval()
    x, pos, ei = t(g["x"]), t(g["pos"]), t(g["edge_index"])
    with torch.no_grad():
        y = m.graph_net(x, pos, ei)
        logits = m((x, pos, ei))  # tuple calling convention of utils/train_model.py:37
    assert max_abs(y, t(g["y"])) < TOL
    assert logits.shape == (2,) and max_abs(logits, t(g["logits"])) < TOL


def test_g5_training_step_matches_reference(G):
    """utils/train_model.py:37-42: forward, CE loss, backward, Adam step."""
    g = load_golden("g5_train_step.npz")
    m = G.CombinedModel(G.GraphNet(**_kwargs(g)), num_nodes=37, classes=2)
    m.load_state_dict(sub_state_dict(g, "before/"), strict=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    sample = (t(g["x"]), t(g["pos"]), t(g["edge_index"]))
    label = t(g["label"])
    logits = m(sample)
    loss = crit(logits, label)
    opt.zero_grad()
    loss.backward()
    assert max_abs(logits.detach(), t(g["logits"])) < TOL
    assert abs(float(loss) - float(g["loss"])) < TOL
    for k, p in m.named_parameters():
        ref = t(g["grad/" + k])
        assert p.grad is not None, k
        assert max_abs(p.grad.cpu(), ref) < 2e-5 + 1e-4 * float(ref.abs().max()), k
    opt.step()
    # one Adam step moves every weight by ~lr*sign(grad); entries whose gradient is at the
    # rounding level can flip sign, so the bound is 2*lr on those and 1e-5 elsewhere
    for k, p in m.state_dict().items():
        ref, gr = t(g["after/" + k]), t(g["grad/" + k]).abs()
        diff = (p.cpu() - ref).abs()
        solid = gr > 1e-5
        assert float(diff[solid].max() if solid.any() else 0) < 2e-5, k
        assert float(diff.max()) <= 2.1e-3, k


def test_block_diagonal_batch_equals_independent_forwards(G):
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(4, seed=1000)  # config C1: ~150-node graphs, batch = 4
    m = G.GraphNet(**S.graphnet_kwargs(64, 2))
    with torch.no_grad():
        y_all = m(batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)).cpu()
        for gi in range(batch.num_graphs):
            s = batch.slice_graphs(gi, gi + 1)
            y = m(s.x.to(DEV), s.pos.to(DEV), s.edge_index.to(DEV)).cpu()
            n0, n1 = int(batch.graph_ptr[gi]), int(batch.graph_ptr[gi + 1])
            assert torch.equal(y, y_all[n0:n1])  # same per-row arithmetic regardless of batching
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    assert max_abs(y_all, O.graphnet_forward(sd, batch.x, batch.pos, batch.edge_index)) < TOL


def test_combined_forward_batched_equals_per_graph(G):
    rng = np.random.default_rng(3)
    n, gcount = 36, 5
    ei1 = torch.from_numpy(O.grid_edge_index(6, 6))
    m = G.CombinedModel(G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=2, out_dim_node=32,
                                   out_dim_edge=32, hidden_dim_node=32, hidden_dim_edge=32, hidden_dim_decoder=32,
                                   hidden_dim_processor_node=32, hidden_dim_processor_edge=32), num_nodes=n, classes=2)
    xs = torch.from_numpy(rng.random((gcount * n, 3)).astype(np.float32))
    rr, cc = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    pos1 = torch.from_numpy(np.stack([rr.ravel(), cc.ravel()], 1).astype(np.float32))
    pos = pos1.repeat(gcount, 1)
    ei = torch.cat([ei1 + k * n for k in range(gcount)], dim=1)
    with torch.no_grad():
        lb = m.forward_batched(xs, pos, ei, gcount)
        for k in range(gcount):
            l1 = m((xs[k * n:(k + 1) * n], pos1, ei1))
            assert max_abs(lb[k], l1) < 2e-6


def test_forward_batched_variable_size_readout_policy(G):
    """graph_ptr mode: first num_nodes nodes feed fc1, smaller graphs are zero-padded (stated deviation; the
    reference's read-out only exists for N == num_nodes)."""
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(5, seed=21)  # 144 / 156 / 169 nodes
    nn_ = 156
    torch.manual_seed(8)
    m = G.CombinedModel(G.GraphNet(**S.graphnet_kwargs(32, 2)), num_nodes=nn_, classes=2)
    w = [p.detach().cpu().double() for fc in (m.classifier.fc1, m.classifier.fc2, m.classifier.fc3) for p in (fc.weight, fc.bias)]
    with torch.no_grad():
        lb = m.forward_batched(batch.x, batch.pos, batch.edge_index, graph_ptr=batch.graph_ptr)
        assert lb.shape == (5, 2)
        for gi in range(5):
            s = batch.slice_graphs(gi, gi + 1)
            y = m.graph_net(s.x, s.pos, s.edge_index).flatten()
            v = torch.zeros(nn_, dtype=torch.float64)
            v[:min(nn_, y.numel())] = y[:nn_].cpu().double()
            # the classifier by formula in float64 on the CPU: m.classifier(v) would be the read-out kernel checking itself
            ref = w[4] @ torch.relu(w[2] @ torch.relu(w[0] @ v + w[1]) + w[3]) + w[5]
            assert max_abs(lb[gi].cpu(), ref) < 2e-6


def test_fused_aggregation_forward_is_bit_identical_to_separate_k1(G, monkeypatch):
    """under no_grad the edge launch forms the node model's aggregate in its epilogue; the forward
    must not change by a single bit against the path with K1 as a separate launch."""
    from graphnet_classifier_amd import synthetic as S
    batch, kw = S.make_workload("c3", scale=0.01)
    torch.manual_seed(11)
    m = G.GraphNet(**kw)
    with torch.no_grad():
        monkeypatch.setattr(G, "FUSED_AGG", True)
        y1 = m(batch.x, batch.pos, batch.edge_index)
        monkeypatch.setattr(G, "FUSED_AGG", False)
        y0 = m(batch.x, batch.pos, batch.edge_index)
    assert torch.equal(y0, y1)
    # with autograd on the separate, differentiable K1 is used and gives the same values
    y2 = m(batch.x, batch.pos, batch.edge_index)
    assert y2.requires_grad and torch.equal(y2.detach(), y0)


def test_k6_folded_into_the_edge_encoder_is_bit_identical(G, monkeypatch):
    """SURVEY 2.2 K6 "prologue of the edge-encoder K4": under no_grad the edge features are computed inside the edge encoder's
    launch (no [E, 4] table); not a bit may change against K6 as its own launch, and with autograd on the stored form runs."""
    from graphnet_classifier_amd import native, synthetic as S
    batch, kw = S.make_workload("c3", scale=0.02)
    torch.manual_seed(12)
    m = G.GraphNet(**kw)
    launches = []
    real = native.edge_features
    monkeypatch.setattr(native, "edge_features", lambda *a: (launches.append(1), real(*a))[1])
    with torch.no_grad():
        y1 = m(batch.x, batch.pos, batch.edge_index)
        assert not launches, "K6 ran as its own launch although the fold serves this shape"
        monkeypatch.setattr(native, "FOLD_EDGE_FEATURES", False)
        y0 = m(batch.x, batch.pos, batch.edge_index)
        assert len(launches) == 1
    assert torch.equal(y0, y1)
    monkeypatch.setattr(native, "FOLD_EDGE_FEATURES", True)
    y2 = m(batch.x, batch.pos, batch.edge_index)  # training form: the backward needs the rows
    assert len(launches) == 2 and y2.requires_grad and torch.equal(y2.detach(), y0)


def test_edge_order_invariance(G):
    """Permuting the edge list changes only the per-destination summation order (fp32 noise)."""
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(3, seed=7)
    m = G.GraphNet(**S.graphnet_kwargs(32, 2))
    p = torch.randperm(batch.num_edges, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        a = m(batch.x, batch.pos, batch.edge_index)
        b = m(batch.x, batch.pos, batch.edge_index[:, p])
    assert max_abs(a, b) < 5e-6


@pytest.mark.parametrize("name,scale", [("c3", 1.0), ("c2", 1.0), ("c5", 1.0)])
def test_full_size_workload_against_oracle_on_sampled_graphs(G, name, scale):
    """BASELINE.json sizes, all at FULL size: the whole batch runs on the GPU; graphs are independent (block
    diagonal), so the oracle checks the first, middle and last graphs of the batch exactly.  At c2 / c5 the
    edge-latent tables are 4.3 GB / 5.12 GB, so the last graphs' edges lie beyond the 4 GiB offset where the
    kernels switch from one whole-table buffer window to a window per tile (csrc/mlp_device.h)."""
    from graphnet_classifier_amd import synthetic as S
    batch, kw = S.make_workload(name, scale)
    torch.manual_seed(11)
    m = G.GraphNet(**kw)
    with torch.no_grad():
        y = m(batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)).cpu()
    assert y.shape == (batch.num_nodes, 1) and bool(torch.isfinite(y).all())
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    ng = batch.num_graphs
    if name != "c3":
        assert batch.num_edges * kw["out_dim_edge"] * 4 > (1 << 32)
    for g0 in (0, ng // 2, ng - 3):
        s = batch.slice_graphs(g0, g0 + 3)
        ref = O.graphnet_forward(sd, s.x, s.pos, s.edge_index)
        n0 = int(batch.graph_ptr[g0])
        assert max_abs(y[n0:n0 + s.num_nodes], ref) < TOL
    # determinism: same inputs, same bits
    with torch.no_grad():
        y2 = m(batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)).cpu()
    assert torch.equal(y, y2)


def test_wsplit_and_reference_form_agree(G, monkeypatch):
    """The algebraic split of the edge processor's first Linear only reorders fp32 sums."""
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(5, seed=3)
    for width in (32, 64, 128):
        torch.manual_seed(width)
        m = G.GraphNet(**S.graphnet_kwargs(width, 2))
        with torch.no_grad():
            monkeypatch.setattr(G, "WSPLIT", True)
            a = m(batch.x, batch.pos, batch.edge_index)
            monkeypatch.setattr(G, "WSPLIT", False)
            b = m(batch.x, batch.pos, batch.edge_index)
        assert max_abs(a, b) < 5e-6
        sd = {k: v.cpu() for k, v in m.state_dict().items()}
        assert max_abs(a, O.graphnet_forward(sd, batch.x, batch.pos, batch.edge_index)) < TOL


def test_hip_backward_agrees_with_torch_recompute_backward(G, monkeypatch):
    """The K8 kernels (data path + skinny GEMMs) against the PyTorch-ROCm recompute backward of the same ops."""
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(6, seed=11)
    x, pos, ei = batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)
    w = torch.randn(batch.num_nodes, 1, device=DEV)
    # six superpixel graphs are a small batch: the fused / weights-resident K8 kernels at 64, the column-split small-batch
    # backward (mlp_bwd_col16.hip) at 128, the 16-row streamed kernel at 256.  The throughput kernels of each width class run
    # in tests/test_gpu_mlp_families.py.
    for width in (64, 128, 256):
        torch.manual_seed(5)
        m = G.GraphNet(**S.graphnet_kwargs(width, 2))
        grads = {}
        for hip in (True, False):
            monkeypatch.setattr(Fn, "HIP_BACKWARD", hip)
            m.zero_grad()
            (m(x, pos, ei) * w).sum().backward()
            grads[hip] = {k: p.grad.clone() for k, p in m.named_parameters()}
        for k in grads[True]:
            a, b = grads[True][k], grads[False][k]
            # Both sides are fp32 with different summation orders (W-split, per-node sums).  A pre-activation within
            # rounding of zero may take the other ReLU branch on one side: that moves single rows' contributions, i.e.
            # a handful of entries by up to ~1e-3 of the largest one, while the tensor as a whole agrees to ~1e-5.
            assert float((a - b).norm() / b.norm().clamp_min(1e-12)) < 1e-3, (width, k)
            assert max_abs(a, b) < 3e-3 * max(1.0, float(b.abs().max())), (width, k)


@pytest.mark.parametrize("case", ["no_edges", "one_node", "self_loops_and_duplicates", "isolated_tail"])
def test_degenerate_graphs(G, case):
    """Empty edge list (the superpixel builder's `np.empty((2, 0))`, superpixel.py:70-71), a single node,
    self loops / repeated edges, and trailing nodes without in-edges."""
    rng = np.random.default_rng(1)
    if case == "no_edges":
        n, ei = 7, torch.zeros(2, 0, dtype=torch.long)
    elif case == "one_node":
        n, ei = 1, torch.tensor([[0, 0], [0, 0]])
    elif case == "self_loops_and_duplicates":
        n, ei = 5, torch.tensor([[0, 0, 0, 1, 1, 3, 3, 3], [0, 1, 1, 1, 2, 3, 4, 4]])
    else:
        n, ei = 9, torch.tensor([[8, 7, 6, 5], [0, 0, 1, 2]])
    x = torch.from_numpy(rng.random((n, 3)).astype(np.float32))
    pos = torch.from_numpy((rng.random((n, 2)) * 10).astype(np.float32))
    torch.manual_seed(2)
    m = G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=2, out_dim_node=32, out_dim_edge=32,
                   hidden_dim_node=32, hidden_dim_edge=32, hidden_dim_decoder=32, hidden_dim_processor_node=32,
                   hidden_dim_processor_edge=32)
    with torch.no_grad():
        y = m(x, pos, ei)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    if case == "no_edges":
        # the reference itself cannot run this graph: MLP.forward's `x.view(x.size(0), -1)` (models/MLP.py:46) is
        # ambiguous for a [0, 3] edge-feature tensor; the engine treats it as "no messages" instead
        with pytest.raises(RuntimeError):
            O.graphnet_forward(sd, x, pos, ei)
        assert y.shape == (n, 1) and bool(torch.isfinite(y).all())
    else:
        ref = O.graphnet_forward(sd, x, pos, ei)
        assert y.shape == ref.shape == (n, 1) and max_abs(y, ref) < TOL
    # and the training direction on the same graph
    y2 = m(x, pos, ei)
    y2.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_captured_forward_replays_bit_identically(G):
    """hipGraph replay of the forward for a fixed pixel-grid topology equals the eager forward, for new inputs."""
    rng = np.random.default_rng(0)
    ei = torch.from_numpy(O.grid_edge_index(16, 16))
    rr, cc = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    pos = torch.from_numpy(np.stack([rr.ravel(), cc.ravel()], 1).astype(np.float32))
    torch.manual_seed(4)
    m = G.CombinedModel(G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=256, classes=2)
    m.eval()
    x0 = torch.from_numpy((rng.random((256, 3)) * 255).astype(np.float32))
    cap = G.CapturedForward(m, x0, pos, ei)
    for _ in range(3):
        x = torch.from_numpy((rng.random((256, 3)) * 255).astype(np.float32))
        with torch.no_grad():
            eager = m((x.to(DEV), pos.to(DEV), ei.to(DEV)))
        assert torch.equal(cap(x).clone(), eager)


def test_captured_forward_for_any_topology_is_bit_identical_to_the_plain_forward(G):
    """CapturedForward(edge_capacity=...): one hipGraph - topology build included - replayed on graphs over the same nodes whose
    edge lists differ in content and length (superpixel graphs); every result equals the eager forward of that graph bit for
    bit (the padding rows only talk to dummy nodes), for the GraphNet alone and with the read-out, default widths."""
    rng = np.random.default_rng(21)
    n = 144
    torch.manual_seed(5)
    gnet = G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3)
    model = G.CombinedModel(gnet, num_nodes=n, classes=2).eval()
    graphs = []
    for _ in range(6):
        e = int(rng.integers(500, 900))
        graphs.append((torch.from_numpy(rng.random((n, 3), dtype=np.float32)), torch.from_numpy((rng.random((n, 2)) * 32).astype(np.float32)),
                       torch.from_numpy(rng.integers(0, n, size=(2, e)).astype(np.int64))))
    for mod in (gnet, model):
        cap = G.CapturedForward(mod, *graphs[0], edge_capacity=1024)
        for k in (1, 2, 3, 4, 5, 0, 3):
            x, pos, ei = graphs[k]
            got = cap(x, pos, ei).clone()
            with torch.no_grad():
                want = mod(x.to(DEV), pos.to(DEV), ei.to(DEV)) if mod is gnet else mod((x.to(DEV), pos.to(DEV), ei.to(DEV)))
            assert got.shape == want.shape and torch.equal(got, want), k
        cap.check()
        x, pos, ei = graphs[1]
        with pytest.raises(ValueError):
            cap(x, pos, torch.cat([ei, ei], dim=1))
        bad = ei.clone()
        bad[0, 3] = n + 2
        with pytest.raises(IndexError):
            cap(x, pos, bad)
        cap(x.to(DEV), pos.to(DEV), bad.to(DEV))
        with pytest.raises(IndexError):
            cap.check()
        bad[0, 3] = 10 ** 6
        out = cap(x.to(DEV), pos.to(DEV), bad.to(DEV))
        assert bool(torch.isnan(out).all())
        with pytest.raises(IndexError):
            cap.check()


def test_captured_forward_for_any_topology_replays_the_general_sort_path(G):
    """Edge lists too long for the LDS topology path (one graph of > 4096 padded edges): every replay runs the general path -
    ONE gated kernel whose passes meet at a grid barrier, its arrival counter re-zeroed inside the graph - and still equals
    the plain forward bit for bit."""
    rng = np.random.default_rng(22)
    n = 300
    torch.manual_seed(6)
    gnet = G.GraphNet(**{**dict(num_local_features=3, space_dim=2, out_channels=1, n_blocks=2), **{k: 32 for k in (
        "out_dim_node", "out_dim_edge", "hidden_dim_node", "hidden_dim_edge", "hidden_dim_decoder", "hidden_dim_processor_node",
        "hidden_dim_processor_edge")}})
    graphs = []
    for _ in range(4):
        e = int(rng.integers(5000, 6000))
        graphs.append((torch.from_numpy(rng.random((n, 3), dtype=np.float32)), torch.from_numpy((rng.random((n, 2)) * 32).astype(np.float32)),
                       torch.from_numpy(rng.integers(0, n, size=(2, e)).astype(np.int64))))
    cap = G.CapturedForward(gnet, *graphs[0], edge_capacity=8192)
    for k in (1, 2, 3, 0, 2):
        x, pos, ei = graphs[k]
        got = cap(x, pos, ei).clone()
        with torch.no_grad():
            want = gnet(x.to(DEV), pos.to(DEV), ei.to(DEV))
        assert torch.equal(got, want), k
    cap.check()


@pytest.mark.parametrize("kw", [
    dict(norm_type=None),
    dict(activation="Tanh"),
    dict(hidden_layers_node=1, hidden_layers_edge=3, hidden_layers_processor_node=3, hidden_layers_processor_edge=1,
         hidden_layers_decoder=1),
    dict(out_dim_node=48, out_dim_edge=24, hidden_dim_node=40, hidden_dim_edge=56, hidden_dim_processor_node=72,
         hidden_dim_processor_edge=36, hidden_dim_decoder=20, out_channels=3),
    dict(num_local_features=5, space_dim=3, num_global_features=2),
    dict(initializer="xavier_uniform_"),
])
def test_graphnet_kwargs_variants_match_oracle(G, kw):
    """Every constructor kwarg of models/GNN.py:230-254 that changes the arithmetic, against the oracle
    (state dict exported from the module, so both sides use the same weights)."""
    rng = np.random.default_rng(len(str(kw)))
    n, e = 120, 700
    nf = kw.get("num_local_features", 3) + kw.get("num_global_features", 0)
    sdim = kw.get("space_dim", 2)
    x = torch.from_numpy(rng.random((n, nf)).astype(np.float32))
    pos = torch.from_numpy((rng.random((n, sdim)) * 16).astype(np.float32))
    ei = torch.from_numpy(rng.integers(0, n, size=(2, e)).astype(np.int64))
    base = dict(n_blocks=2, out_dim_node=32, out_dim_edge=32, hidden_dim_node=32, hidden_dim_edge=32,
                hidden_dim_decoder=32, hidden_dim_processor_node=32, hidden_dim_processor_edge=32)
    base.update(kw)
    torch.manual_seed(3)
    m = G.GraphNet(**base)
    with torch.no_grad():
        y = m(x, pos, ei)
    if kw.get("activation") == "Tanh":
        # the oracle restates ReLU only (the reference never uses another activation); check against torch modules
        ref_mod = {k: v.cpu() for k, v in m.state_dict().items()}
        import torch.nn.functional as F

        def mlp(prefix, t, ln=True):
            idx = sorted({int(k[len(prefix) + 7:].split(".")[0]) for k in ref_mod if k.startswith(prefix + ".model.")})
            lin = [i for i in idx if ref_mod[f"{prefix}.model.{i}.weight"].ndim == 2]
            for q, i in enumerate(lin):
                t = F.linear(t, ref_mod[f"{prefix}.model.{i}.weight"], ref_mod[f"{prefix}.model.{i}.bias"])
                if q + 1 < len(lin):
                    t = torch.tanh(t) if "decoder" not in prefix else torch.relu(t)  # decoder keeps the default ReLU (:289-295)
            nrm = [i for i in idx if ref_mod[f"{prefix}.model.{i}.weight"].ndim == 1]
            for i in nrm:
                t = F.layer_norm(t, (t.size(-1),), ref_mod[f"{prefix}.model.{i}.weight"], ref_mod[f"{prefix}.model.{i}.bias"])
            return t
        ef = O.edge_features(pos, ei)
        hh, ee = mlp("node_encoder", x), mlp("edge_encoder", ef)
        for b in range(2):
            p = f"graph_processor.blocks.{b}"
            ee = mlp(p + ".edge_model.edge_processor", torch.cat([hh[ei[0]], hh[ei[1]], ee], -1)) + ee
            agg = O.scatter_sum_fast(ee, ei[1], n)
            hh = mlp(p + ".node_model.node_processor", torch.cat([hh, agg], -1)) + hh
        ref = mlp("node_decoder", hh)
    else:
        ref = O.graphnet_forward({k: v.cpu() for k, v in m.state_dict().items()}, x, pos, ei)
    assert y.shape == ref.shape and max_abs(y, ref) < 2e-5


def test_batchnorm_norm_type_runs_through_the_kernel_plus_a_rocm_op(G):
    """norm_type='BatchNorm1d' is legal in models/MLP.py:30-35 (never used by the reference's entry points)."""
    from graphnet_classifier_amd.MLP import MLP
    torch.manual_seed(0)
    m = MLP(12, 20, hidden_dim=32, hidden_layers=2, norm_type="BatchNorm1d")
    x = torch.randn(50, 12)
    ref = torch.nn.Sequential(*[type(l)(**({"in_features": l.in_features, "out_features": l.out_features} if isinstance(l, torch.nn.Linear)
                                             else {"num_features": l.num_features} if isinstance(l, torch.nn.BatchNorm1d) else {}))
                                for l in m.model])
    ref.load_state_dict({k: v.cpu() for k, v in m.model.state_dict().items()})
    for mode in ("train", "eval"):
        getattr(m, mode)(); getattr(ref, mode)()
        with torch.no_grad():
            assert max_abs(m(x), ref(x)) < 2e-5


def test_bench_two_ranks_rehearsal_on_one_gpu(tmp_path):
    """bench.py's N > 1 bookkeeping (rank-local batches, barrier + max-over-ranks timing, summed units, one JSON
    line on rank 0) with two ranks sharing this GPU over gloo; the real runs use RCCL, one rank per GPU.  The default
    at N > 1 is BASELINE config c4 (the c3 graphs split by graph id, strong scaling) with a training leg whose step
    holds exactly ONE collective."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GNC_BENCH_BACKEND="gloo")
    for extra, graphs, scaling in (([], 62, "strong"), (["--scaling", "weak"], 2 * 62, "weak"), (["--mode", "train"], 62, "strong")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", "29531", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup",
               "1", "--scale", "0.01", "--full", "--no-cpu-baseline", "--train-steps", "2"] + extra
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert out.returncode == 0 and len(lines) == 1, out.stderr[-2000:]
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["config"]["graphs"] == graphs and d["value"] > 0
        assert d["scaling"] == scaling
        if scaling == "strong":
            assert d["config"]["workload"].startswith("c4:"), d["config"]["workload"]
        if "--mode" not in extra:  # N > 1: the forward step is replayed from one hipGraph (small shards are launch-bound)
            assert d["step_launch"].startswith("one hipGraph replay"), d["step_launch"]
        tr = d["train"]
        # the training step too: forward + CE + backward + gradient pack replayed, then ONE collective and the Adam launch
        assert tr["step_launch"].startswith("one hipGraph replay"), tr["step_launch"]
        assert tr["collectives_per_step"] == 1.0 and tr["allreduce_ms"] > 0 and tr["value"] > 0
        assert tr["allreduce_bytes"] >= 4 * 60_000


def test_bench_plain_run_dumps_the_last_timed_output(G, tmp_path):
    """A plain bench.py run measures the headline figure only, and --dump-outputs holds the forward of the timed step:
    the oracle's result for the same seeded batch and weights."""
    import json
    import os
    import subprocess
    import sys
    from graphnet_classifier_amd import synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--scale", "0.01",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f32"
    assert not {"roofline", "kernel_ms_per_step", "train", "topology_cached", "cpu_baseline"} & set(d)
    assert os.listdir(tmp_path) == ["output.npy"]
    y = np.load(tmp_path / "output.npy")
    batch, kw = synthetic.make_workload("c3", 0.01)
    assert y.dtype == np.float32 and y.shape == (batch.num_nodes, 1) == (d["config"]["nodes"], 1)
    torch.manual_seed(0)  # bench.py's weights
    sd = {k: v.detach().cpu() for k, v in G.GraphNet(**kw).state_dict().items()}
    s = batch.slice_graphs(0, 3)
    with torch.no_grad():
        ref = O.graphnet_forward(sd, s.x, s.pos, s.edge_index)
    assert max_abs(torch.from_numpy(y[: s.num_nodes]), ref) < TOL


def test_forward_on_cpu_module_fails_loudly(G):
    m = G.GraphNet(**{"n_blocks": 1}).to("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(2, 3, dtype=torch.long))


def test_deferred_validation_poisons_the_output_and_raises_at_the_check(G):
    """topology.set_validation("deferred"): no host sync in the build; a bad edge_index gives NaN on the device and
    the IndexError of the synchronous mode when check_deferred() is called."""
    from graphnet_classifier_amd import synthetic as S
    from graphnet_classifier_amd import topology
    batch = S.superpixel_like_graphs(2, seed=4)
    torch.manual_seed(1)
    m = G.GraphNet(**S.graphnet_kwargs(32, 1))
    x, pos, ei = batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)
    with torch.no_grad():
        ref = m(x, pos, ei)
    bad = ei.clone()
    bad[0, 5] = batch.num_nodes + 3
    with pytest.raises(IndexError):
        with torch.no_grad():
            m(x, pos, bad)  # default mode: raised by the build
    topology.set_validation("deferred")
    try:
        topology.clear_topology_cache()
        with torch.no_grad():
            good = m(x, pos, ei)
            poisoned = m(x, pos, bad)
        assert torch.equal(good, ref)
        assert bool(torch.isnan(poisoned).all())
        with pytest.raises(IndexError):
            topology.check_deferred()
        topology.check_deferred()  # nothing pending any more
        # the block-level entry points build a topology too: same rule (advisor finding of round 2)
        block = m.graph_processor.blocks[0]
        xn = torch.randn(batch.num_nodes, 32, device=DEV)
        ea = torch.randn(ei.size(1), 32, device=DEV)
        for grad in (False, True):
            with torch.set_grad_enabled(grad):
                topology.clear_topology_cache()
                outs = list(block(xn, bad, ea)[:2]) + list(m.graph_processor(xn, bad, ea)) + [block.node_model(xn, bad, ea)]
                assert all(bool(torch.isnan(o).all()) for o in outs)
                okx, oke, _ = block(xn, ei, ea)
                assert bool(torch.isfinite(okx).all()) and bool(torch.isfinite(oke).all())
            with pytest.raises(IndexError):
                topology.check_deferred()
    finally:
        topology.set_validation("sync")
        topology.clear_topology_cache()


@pytest.mark.parametrize("width", [40, 96, 160, 200])
def test_hip_backward_odd_widths_agree_with_torch_recompute_backward(G, monkeypatch, width):
    """Widths that are not a multiple of 64 (tails of the 64-column chunks, partial accumulator tiles) through the K8 kernels
    a batch of four superpixel graphs reaches - the fused / weights-resident kernels (40), the column-split small-batch
    backward (96), the 16-row streamed kernel (160, 200) - against the PyTorch-ROCm recompute backward of the same ops.  The
    throughput kernels of each width class run in tests/test_gpu_mlp_families.py."""
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(4, seed=width)
    x, pos, ei = batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)
    w = torch.randn(batch.num_nodes, 1, device=DEV)
    torch.manual_seed(width)
    m = G.GraphNet(**S.graphnet_kwargs(width, 2))
    grads = {}
    for hip in (True, False):
        monkeypatch.setattr(Fn, "HIP_BACKWARD", hip)
        m.zero_grad()
        (m(x, pos, ei) * w).sum().backward()
        grads[hip] = {k: p.grad.clone() for k, p in m.named_parameters()}
    for k in grads[True]:
        a, b = grads[True][k], grads[False][k]
        assert float((a - b).norm() / b.norm().clamp_min(1e-12)) < 1e-3, (width, k)
        assert max_abs(a, b) < 3e-3 * max(1.0, float(b.abs().max())), (width, k)


@pytest.mark.parametrize("out_edge,hidden", [(30, 32), (30, 64), (22, 48)])
def test_hip_backward_edge_width_not_a_multiple_of_four(G, monkeypatch, out_edge, hidden):
    """Edge latents whose width is not a multiple of 4 reach the kernels through a zero-padded copy, so the residual is
    NOT the staged segment and its gradient (the effective output gradient: rows + the aggregation's gathered part) has
    to be added by the caller: the W-split backward must then get that sum as a tensor (advisor finding, round 2)."""
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(3, seed=out_edge)
    x, pos, ei = batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV)
    w = torch.randn(batch.num_nodes, 1, device=DEV)
    torch.manual_seed(out_edge + hidden)
    m = G.GraphNet(n_blocks=2, out_dim_node=32, out_dim_edge=out_edge, hidden_dim_node=32, hidden_dim_edge=hidden,
                   hidden_dim_decoder=32, hidden_dim_processor_node=32, hidden_dim_processor_edge=hidden)
    grads = {}
    for hip in (True, False):
        monkeypatch.setattr(Fn, "HIP_BACKWARD", hip)
        m.zero_grad()
        (m(x, pos, ei) * w).sum().backward()
        grads[hip] = {k: p.grad.clone() for k, p in m.named_parameters()}
    for k in grads[True]:
        a, b = grads[True][k], grads[False][k]
        assert float((a - b).norm() / b.norm().clamp_min(1e-12)) < 1e-3, (k,)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        assert max_abs(m(x, pos, ei).cpu(), O.graphnet_forward(sd, batch.x, batch.pos, batch.edge_index)) < TOL


def test_g9_default_model_gradients_match_reference(G):
    """The default-width (128, 3 blocks: main.py:72-73) training step on the R = 32 pixel graph: logits, loss and all
    76 parameter gradients against what the reference's own classes produced (golden G9).  This is the pin of the
    128-wide K8 kernels (streamed weights, 32-row tiles, 2-wave small-batch instances) against reference gradients."""
    g = load_golden("g9_default_train_grads.npz")
    m = G.CombinedModel(G.GraphNet(num_local_features=3, space_dim=2, out_channels=1, n_blocks=3), num_nodes=1024, classes=2)
    m.load_state_dict(sub_state_dict(g, "before/"), strict=True)
    logits = m((t(g["x"]), t(g["pos"]), t(g["edge_index"])))
    loss = torch.nn.CrossEntropyLoss()(logits, t(g["label"]))
    m.zero_grad()
    loss.backward()
    assert max_abs(logits.detach(), t(g["logits"])) < TOL
    assert abs(float(loss) - float(g["loss"])) < TOL
    # Noise floor of this comparison: the reference's fp32 gradients differ from an fp64 run of the same model by up to
    # 9.7e-3 of a tensor's largest entry (blocks.1 edge processor, second Linear): a pre-activation within rounding of
    # zero takes the other ReLU branch, which moves one row's whole contribution.  The HIP path sums in another order
    # (W-split, MFMA k-order), so it sits at the same kind of distance: entries are compared at rounding level, and the
    # few that a flipped unit moves are bounded tensor-wise.
    close = total = 0
    for k, p in m.named_parameters():
        ref = t(g["grad/" + k])
        assert p.grad is not None, k
        got = p.grad.cpu()
        tol = 2e-5 + 1e-4 * float(ref.abs().max())
        close += int(((got - ref).abs() < tol).sum())
        total += ref.numel()
        assert float((got - ref).norm() / ref.norm().clamp_min(1e-12)) < 2e-2, (k, float((got - ref).norm() / ref.norm()))
        assert max_abs(got, ref) < 2e-5 + 3e-2 * float(ref.abs().max()), (k, max_abs(got, ref), float(ref.abs().max()))
    assert close / total > 0.995, close / total
    assert len(list(m.named_parameters())) == 76


@pytest.mark.parametrize("name", ["c2", "c5"])
def test_full_size_backward_against_oracle_autograd_on_sampled_graphs(G, name):
    """BASELINE sizes, backward: `(y * w).sum().backward()` over the FULL batch (c2: 10k graphs at width 128, c5: 500k
    nodes / 5M edges at width 256; edge tables beyond 4 GiB) with `x.requires_grad_()`.  The batch is block diagonal, so
    the input gradient of a graph depends on that graph alone: the rows of x.grad that belong to the first, middle and
    last graphs are checked against the oracle's CPU autograd on those graphs (the oracle's autograd is pinned by the
    reference's own gradients in test_oracle_golden.py, goldens G5 / G9), plus bitwise run-to-run reproducibility."""
    from graphnet_classifier_amd import synthetic as S
    batch, kw = S.make_workload(name, 1.0)
    torch.manual_seed(13)
    m = G.GraphNet(**kw)
    wgt = torch.randn(batch.num_nodes, 1, generator=torch.Generator().manual_seed(5))
    pos, ei = batch.pos.to(DEV), batch.edge_index.to(DEV)
    wd = wgt.to(DEV)
    grads = []
    for _ in range(2):
        x = batch.x.to(DEV).requires_grad_(True)
        m.zero_grad(set_to_none=True)
        (m(x, pos, ei) * wd).sum().backward()
        grads.append(x.grad.cpu())
        del x
    assert torch.equal(grads[0], grads[1])
    assert batch.num_edges * kw["out_dim_edge"] * 4 > (1 << 32)
    gx = grads[0]
    assert bool(torch.isfinite(gx).all())
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ng = batch.num_graphs
    tight = []
    for g0 in (0, ng // 2, ng - 3):
        s = batch.slice_graphs(g0, g0 + 3)
        n0 = int(batch.graph_ptr[g0])
        xs = s.x.clone().requires_grad_(True)
        O.set_scatter_impl("index_add")  # the differentiable restatement of models/GNN.py:18-20
        try:
            (O.graphnet_forward(sd, xs, s.pos, s.edge_index) * wgt[n0:n0 + s.num_nodes]).sum().backward()
        finally:
            O.set_scatter_impl("sorted_loop")
        ref = xs.grad
        got = gx[n0:n0 + s.num_nodes]
        # a pre-activation within rounding of zero may take the other ReLU branch on one side (different fp32 summation
        # orders; the same happens between the reference's fp32 and an fp64 run of it, see the G9 test): every input
        # gradient of THAT graph then moves by a visible amount, the other graphs agree at rounding level.  So: every
        # graph within the loose bounds, and most of the sampled graphs entirely within the tight one.
        tol = 2e-5 + 1e-4 * float(ref.abs().max())
        assert float((got - ref).norm() / ref.norm().clamp_min(1e-12)) < 1e-2, (name, g0)
        assert max_abs(got, ref) < 2e-5 + 5e-2 * float(ref.abs().max()), (name, g0)
        for k in range(3):
            a, b = int(s.graph_ptr[k]), int(s.graph_ptr[k + 1])
            tight.append(bool(((got[a:b] - ref[a:b]).abs() < tol).all()))
    assert sum(tight) >= 6, tight  # 9 sampled graphs


@pytest.mark.parametrize("act", ["Tanh", "SiLU", "GELU", "LeakyReLU", "ELU", "Sigmoid"])
def test_training_with_another_activation_runs_on_the_library_and_matches_autograd(G, monkeypatch, act):
    """models/MLP.py:21 accepts any nn.<Name>.  For an activation other than ReLU the backward runs layer by layer on the
    library's own kernels (functional._layerwise_mlp_backward_hip: single-Linear K4 launches, csrc/elementwise.hip, xty):
    parameter and input gradients against the PyTorch-ROCm recompute backward of the same ops, and no silent switch to it."""
    from graphnet_classifier_amd import functional as Fn
    from graphnet_classifier_amd import synthetic as S
    batch = S.superpixel_like_graphs(3, seed=9)
    pos, ei = batch.pos.to(DEV), batch.edge_index.to(DEV)
    w = torch.randn(batch.num_nodes, 1, device=DEV)
    torch.manual_seed(4)
    m = G.GraphNet(n_blocks=2, out_dim_node=32, out_dim_edge=32, hidden_dim_node=32, hidden_dim_edge=32, hidden_dim_decoder=32,
                   hidden_dim_processor_node=32, hidden_dim_processor_edge=32, activation=act)
    calls = []
    real = Fn._layerwise_mlp_backward_hip
    monkeypatch.setattr(Fn, "_layerwise_mlp_backward_hip", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    grads = {}
    for hip in (True, False):
        monkeypatch.setattr(Fn, "HIP_BACKWARD", hip)
        x = batch.x.to(DEV).requires_grad_(True)
        m.zero_grad()
        (m(x, pos, ei) * w).sum().backward()
        grads[hip] = dict({k: p.grad.clone() for k, p in m.named_parameters()}, x=x.grad.clone())
    assert len(calls) >= 6  # both encoders and the two blocks' processors (the decoder keeps ReLU: models/GNN.py:289-295)
    for k in grads[True]:
        a, b = grads[True][k], grads[False][k]
        assert max_abs(a, b) < 2e-5 + 1e-4 * float(b.abs().max()), (k, max_abs(a, b), float(b.abs().max()))
