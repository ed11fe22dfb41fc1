"""GPU: ``CombinedModel(readout="attention")`` - the attention read-out (K19) through every caller of
``CombinedModel.readout_logits`` - against the CPU oracle (``O.graphnet_forward``, the gate by ``O.mlp_forward``, a torch softmax,
``O.classifier_forward``), its gradients against float64 autograd of the same path, the captures against the eager steps, and the
untouched defaults.  Graphs: the superpixel fixtures of tests/golden/g10_superpixel*.npz with 69, 100 and 119 nodes (and three more
for the batches).  GraphNet: ``synthetic.graphnet_kwargs(64, 2, out_channels=8)``, seeded.

The freshly initialised gate is almost uniform at this seed (an implementation that silently took the mean would pass at 1e-5), so
every model of this file has ``gate.model.2.weight`` multiplied by ``SHARPEN`` in place before anything is computed, and
``test_the_sharpened_gate_is_far_from_the_mean`` asserts in the float64 reference alone that the attention logits then differ from
the mean-pooling logits of the same parameters by at least ten bars on each graph (the figures are in DESIGN.md, K19)."""
import numpy as np
import pytest
import torch

from oracle import graphnet_oracle as O
from oracle import image_graph_oracle as IO
from tests._util import max_abs
from tests.test_superpixel_golden import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234
OUT_DIM = 8
SHARPEN = 100.0
THREE = ((20, 69), (10, 119), (35, 100))  # (case id, nodes): the smallest, the largest, then num_nodes itself
SIX = (10, 20, 8, 13, 35, 31)


def _graph(case_id):
    """Fixture graph of a case as CPU tensors (the reference's where the fixture has it, else the oracle's build)."""
    _, img, labels, _, graph = CASES[case_id]
    assert CASES[case_id][0] == case_id
    if graph is None:
        graph = IO.superpixel_graph_from_labels(img, labels)
    x, pos, ei = (torch.from_numpy(np.ascontiguousarray(np.asarray(a))) for a in graph)
    return x.float(), pos.float(), ei.long()


def _model(readout="attention", num_nodes=100, **extra):
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    torch.manual_seed(SEED)
    gnet = GraphNet(**synthetic.graphnet_kwargs(64, 2, out_channels=OUT_DIM))
    if readout is None:
        return CombinedModel(gnet, num_nodes, 2)  # the constructor call of before the read-out argument
    m = CombinedModel(gnet, num_nodes=num_nodes, classes=2, readout=readout, **extra)
    if readout == "attention":
        with torch.no_grad():
            m.gate.model[2].weight.mul_(SHARPEN)
    return m


def _oracle(sd, x, pos, ei, pooling="attention"):
    """(logits, alpha) of the oracle path in the dtype of ``sd``; ``pooling="mean"``: the mean of the same node outputs instead."""
    y = O.graphnet_forward(sd, x, pos, ei, prefix="graph_net.")
    alpha = torch.softmax(O.mlp_forward(sd, "gate", y)[:, 0], dim=0)
    pooled = alpha @ y if pooling == "attention" else y.mean(0)
    return O.classifier_forward(sd, pooled), alpha


def sharpened_gate_figures():
    """[(nodes, |attention - mean logits| in float64, max alpha n, |fp32 oracle - float64 oracle|)]: needs no GPU (construction works
    on the CPU), so it can be run before the first GPU run; the figures at this seed are in DESIGN.md, K19."""
    sd = {k: v.detach().cpu() for k, v in _model().state_dict().items()}
    sd64 = O.to_dtype(sd, torch.float64)
    out = []
    for case_id, nodes in THREE:
        x, pos, ei = _graph(case_id)
        att, alpha = _oracle(sd64, x.double(), pos.double(), ei)
        mean, _ = _oracle(sd64, x.double(), pos.double(), ei, pooling="mean")
        l32, _ = _oracle(sd, x, pos, ei)
        out.append((nodes, max_abs(att, mean), float(alpha.max()) * nodes, max_abs(l32, att)))
    return out


@pytest.fixture(scope="module")
def graphs():
    return {case_id: _graph(case_id) for case_id in sorted(set(SIX) | {c for c, _ in THREE})}


@pytest.fixture(scope="module")
def collate():
    from graphnet_classifier_amd.image_to_graph import collate_graphs
    return collate_graphs


def test_the_sharpened_gate_is_far_from_the_mean():
    """A condition on the test's inputs, in the float64 reference alone: ten bars between attention and mean pooling on each graph,
    and the fp32 oracle within half a bar of the float64 one."""
    for nodes, apart, peak, fp32 in sharpened_gate_figures():
        print(f"{nodes} nodes: |attention - mean logits| = {apart:.2e}, max alpha n = {peak:.2f}, |fp32 - float64 oracle| = {fp32:.1e}")
        assert apart >= 1e-4 and fp32 <= 5e-6


def test_logits_match_the_oracle_single_and_batched(graphs, collate):
    m = _model().eval()
    assert m.classifier.fc1.in_features == OUT_DIM and m.ragged_readout and m.pooled
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    batch = collate([graphs[c] for c, _ in THREE])
    with torch.no_grad():
        batched = m.forward_batched(batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV), graph_ptr=batch.graph_ptr).cpu()
    assert batched.shape == (3, 2)
    for g, (case_id, nodes) in enumerate(THREE):
        x, pos, ei = graphs[case_id]
        assert x.size(0) == nodes
        ref, _ = _oracle(sd, x, pos, ei)
        with torch.no_grad():
            logits = m((x.to(DEV), pos.to(DEV), ei.to(DEV))).cpu()
        print(f"{nodes} nodes: |forward - oracle| = {max_abs(logits, ref):.3e}, |forward_batched - oracle| = {max_abs(batched[g], ref):.3e}")
        assert logits.shape == (2,) and max_abs(logits, ref) <= 1e-5
        assert max_abs(batched[g], ref) <= 1e-5


def test_num_graphs_form_and_rows_behind_the_graphs(graphs):
    """``forward_batched(num_graphs=G)``: graph g owns rows [g num_nodes, (g + 1) num_nodes); and a ``graph_ptr`` that ends in
    front of the last rows ignores them."""
    x, pos, ei = (t.to(DEV) for t in graphs[35])  # 100 nodes
    m = _model(num_nodes=100).eval()
    xx, pp, ee = torch.cat([x, x.flip(0)]), torch.cat([pos, pos.flip(0)]), torch.cat([ei, 199 - ei], dim=1)
    with torch.no_grad():
        one = m((x, pos, ei))
        two = m.forward_batched(xx, pp, ee, num_graphs=2)
        first = m.forward_batched(xx, pp, ee, graph_ptr=torch.tensor([0, 100]))
    assert two.shape == (2, 2) and max_abs(two[0], one) <= 1e-5 and max_abs(two[1], one) <= 1e-5  # the mirrored graph is a relabelling
    assert first.shape == (1, 2) and max_abs(first[0], one) <= 1e-5


def test_relabelling_the_nodes_leaves_the_logits_alone(graphs):
    x, pos, ei = graphs[10]
    n = x.size(0)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))  # new id k holds old node perm[k]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    xp, pp, eip = x[perm], pos[perm], inv[ei]
    m = _model().eval()
    with torch.no_grad():
        a = m((x.to(DEV), pos.to(DEV), ei.to(DEV)))
        b = m((xp.to(DEV), pp.to(DEV), eip.to(DEV)))
        wa, wb = m.attention_weights(x.to(DEV), pos.to(DEV), ei.to(DEV)), m.attention_weights(xp.to(DEV), pp.to(DEV), eip.to(DEV))
    print(f"relabelled 119-node graph: attention logits move by {max_abs(a, b):.3e}, weights by {max_abs(wa[perm], wb):.3e}")
    assert max_abs(a, b) <= 1e-5 and max_abs(wa[perm], wb) <= 1e-6


def _reference_gradients(m, x, pos, ei, label):
    """float64 autograd of the oracle forward + gate + softmax pooling + dense layers on the CPU."""
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    O.set_scatter_impl("index_add")  # the differentiable ATen form of the same sum
    try:
        logits, _ = _oracle(sd, x.double(), pos.double(), ei)
    finally:
        O.set_scatter_impl("sorted_loop")
    torch.nn.functional.cross_entropy(logits[None], label[None]).backward()
    return {k: v.grad for k, v in sd.items()}


def _assert_gradients(got, ref, what):
    for k, r in ref.items():
        tol = 2e-5 + 1e-4 * float(r.abs().max())
        err = max_abs(got[k].cpu(), r.cpu())
        assert got[k].shape == r.shape and err <= tol, f"{what}: {k} err {err:.3e} > {tol:.3e}"


GATE = ("gate.model.0.weight", "gate.model.0.bias", "gate.model.2.weight", "gate.model.2.bias")


def test_gradients_against_float64_autograd(graphs):
    x, pos, ei = graphs[20]
    label = torch.tensor(1)
    m = _model()
    torch.nn.CrossEntropyLoss()(m((x.to(DEV), pos.to(DEV), ei.to(DEV))), label.to(DEV)).backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    ref = _reference_gradients(m, x, pos, ei, label)
    assert set(ref) == set(got) and set(GATE) <= set(got) and bool(got["graph_net.node_encoder.model.0.weight"].any())
    for k in GATE:
        assert bool(got[k].any()) and bool(ref[k].any()), k
    _assert_gradients(got, ref, "eager attention step")


def _eager_loss_and_gradients(state_dict, forward, label):
    """Loss and gradients of ONE eager step from the given parameters."""
    e = _model()
    e.load_state_dict(state_dict)
    loss = torch.nn.CrossEntropyLoss()(forward(e), label.to(DEV))
    loss.backward()
    return float(loss.item()), {k: p.grad.clone() for k, p in e.named_parameters()}


def test_captured_train_step_over_a_node_capacity_equals_eager_steps(graphs):
    """Three replays over graphs of 69 / 119 / 100 nodes; each step's loss (1e-5) and gradients (2e-5 + 1e-4 max|ref|) against the
    eager step from the parameters the replay started from."""
    from graphnet_classifier_amd.train import CapturedTrainStep, FlatParameters, FusedAdam
    crit = torch.nn.CrossEntropyLoss()
    m = _model()
    fp = FlatParameters(m)
    assert set(GATE) <= set(fp.names)  # picked up by name
    opt = FusedAdam(fp)
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = CapturedTrainStep(m, opt, crit, graphs[10], torch.tensor(0), loss_sum, edge_capacity=1024, node_capacity=128)
    torch.cuda.synchronize()
    assert float(loss_sum.item()) == 0.0 and all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert step.x.size(0) == 128 + 128  # node slots + dummies: num_nodes sizes nothing on a pooled model
    seen = 0.0
    for (case_id, nodes), label in zip(THREE, (torch.tensor(1), torch.tensor(0), torch.tensor(1))):
        sample = graphs[case_id]
        start = {k: v.detach().clone() for k, v in m.state_dict().items()}
        loss, want = _eager_loss_and_gradients(start, lambda e: e(tuple(t.to(DEV) for t in sample)), label)
        assert step.matches(sample)
        step(sample, label)
        step.check()
        torch.cuda.synchronize()
        total = float(loss_sum.item())
        print(f"{nodes} nodes: captured loss {total - seen:.8f}, eager {loss:.8f}")
        assert abs((total - seen) - loss) <= 1e-5
        seen = total
        _assert_gradients(dict(zip(opt.fp.names, opt.fp.reducer.views)), want, f"captured step on {nodes} nodes")
        assert any(not torch.equal(start[k], v) for k, v in m.state_dict().items())


def test_captured_forward_over_a_node_capacity_equals_eager(graphs):
    from graphnet_classifier_amd.GNN import CapturedForward
    m = _model().eval()
    on_dev = {c: tuple(t.to(DEV) for t in graphs[c]) for c, _ in THREE}
    first = THREE[0][0]
    cap = CapturedForward(m, *on_dev[first], edge_capacity=1024, node_capacity=128)
    for c, _ in THREE:
        with torch.no_grad():
            want = m(on_dev[c])
        assert max_abs(cap(*on_dev[c]), want) <= 1e-5, c
    cap.check()
    fixed = CapturedForward(m, *on_dev[35])  # one fixed topology: graph_ptr = [0, N]
    with torch.no_grad():
        assert max_abs(fixed(on_dev[35][0], on_dev[35][1]), m(on_dev[35])) <= 1e-5
    same_nodes = CapturedForward(m, *on_dev[35], edge_capacity=1024)  # any topology over the same node count
    with torch.no_grad():
        assert max_abs(same_nodes(*on_dev[35]), m(on_dev[35])) <= 1e-5


def test_captured_ragged_batch_step_equals_eager_steps(graphs, collate):
    """Two batches of 3 graphs; per step the bars of tests/test_gpu_ragged_batch_capture.py: loss 1e-5, gradients
    2e-5 + 1e-4 max|ref|, against the eager ``forward_batched`` step from the parameters the replay started from."""
    from graphnet_classifier_amd.train import CapturedRaggedBatchStep, FlatParameters, FusedAdam, padded_capacity
    crit = torch.nn.CrossEntropyLoss()
    batches = [collate([graphs[c] for c in SIX[:3]]), collate([graphs[c] for c in SIX[3:]])]
    labels = [torch.tensor([0, 1, 1]), torch.tensor([1, 0, 1])]
    assert batches[0].num_nodes != batches[1].num_nodes
    E = padded_capacity(max(b.num_edges for b in batches))
    M = padded_capacity(max(b.num_nodes for b in batches), 0, 32)
    m = _model()
    opt = FusedAdam(FlatParameters(m))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    step = CapturedRaggedBatchStep(m, opt, crit, batches[0].to(DEV), labels[0], loss_sum, edge_capacity=E, node_capacity=M)
    torch.cuda.synchronize()
    assert float(loss_sum.item()) == 0.0 and int(opt.step_count.item()) == 0
    seen = 0.0
    for b, lab in zip(reversed(batches), reversed(labels)):  # the other batch first
        start = {k: v.detach().clone() for k, v in m.state_dict().items()}
        loss, want = _eager_loss_and_gradients(
            start, lambda e: e.forward_batched(b.x.to(DEV), b.pos.to(DEV), b.edge_index.to(DEV), graph_ptr=b.graph_ptr), lab)
        step(b.to(DEV), lab)
        step.check()
        torch.cuda.synchronize()
        total = float(loss_sum.item())
        print(f"{b.num_nodes} nodes: captured loss {total - seen:.8f}, eager {loss:.8f}")
        assert abs((total - seen) - loss) <= 1e-5
        seen = total
        _assert_gradients(dict(zip(opt.fp.names, opt.fp.reducer.views)), want, f"captured batch step on {b.num_nodes} nodes")
    assert int(opt.step_count.item()) == 2


def test_evaluate_and_predict_captured_equal_eager(graphs, collate):
    from graphnet_classifier_amd.train import evaluate, predict
    m = _model().eval()
    loader = [(collate([graphs[a], graphs[b]]), torch.tensor([k % 2, (k + 1) % 2])) for k, (a, b) in enumerate(zip(SIX[0::2], SIX[1::2]))]
    ev_c, ev_e = evaluate(m, loader, capture=True), evaluate(m, loader, capture=False)
    assert ev_c["count"] == ev_e["count"] == 6 and torch.equal(ev_c["confusion"], ev_e["confusion"])
    assert abs(ev_c["loss"] - ev_e["loss"]) <= 1e-5
    (logits_c, prob_c), (logits_e, prob_e) = predict(m, loader, capture=True), predict(m, loader, capture=False)
    assert logits_c.shape == logits_e.shape == (6, 2)
    print(f"attention predict: max |captured - eager| = {max_abs(logits_c, logits_e):.3e}")
    assert max_abs(logits_c, logits_e) <= 1e-5 and max_abs(prob_c, prob_e) <= 1e-5


def test_attention_weights(graphs):
    m = _model().eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for case_id, nodes in THREE:
        x, pos, ei = graphs[case_id]
        _, ref = _oracle(sd, x, pos, ei)
        w = m.attention_weights((x.to(DEV), pos.to(DEV), ei.to(DEV)))  # the tuple form
        assert w.shape == (nodes,) and w.device.type == "cuda" and not w.requires_grad
        assert max_abs(w.cpu(), ref) <= 1e-6 and abs(float(w.double().sum()) - 1.0) <= 1e-5
    x, pos, ei = graphs[35]
    on_cpu = m.attention_weights(x, pos, ei)  # inputs on the CPU: the result comes back there
    assert on_cpu.device.type == "cpu" and max_abs(on_cpu, w.cpu()) <= 1e-6
    with pytest.raises(ValueError):
        _model("mean").attention_weights(x.to(DEV), pos.to(DEV), ei.to(DEV))


def test_the_defaults_are_untouched(graphs):
    """``readout="mean"`` and the default flatten model: no gate, and the same logits bit for bit from two constructions at one
    seed; the attention model shares every non-gate parameter with the mean model."""
    x, pos, ei = (t.to(DEV) for t in graphs[35])  # 100 nodes
    for readout in ("mean", None):
        a, b = _model(readout).eval(), _model(readout).eval()
        assert not hasattr(a, "gate") and not any(k.startswith("gate") for k in a.state_dict())
        with torch.no_grad():
            assert torch.equal(a((x, pos, ei)), b((x, pos, ei)))
    mean, att = _model("mean").state_dict(), _model().state_dict()
    assert all(torch.equal(att[k], v) for k, v in mean.items())
    with pytest.raises(ValueError):
        _model("mean", gate_hidden=16)
