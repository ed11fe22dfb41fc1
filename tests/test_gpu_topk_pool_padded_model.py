"""GPU: ``GraphNet(pool_ratio=0.5, pool_padded=True)`` - the capacity-padded top-K pooling layers (K20), which read nothing back - under
``CombinedModel`` read-outs ``"mean"`` and ``"attention"``: eager against the composed oracle of tests/topk_pool_cases.py and against
float64 autograd, crossed with the aggregations, and through every capture (``CapturedForward`` in its three forms,
``CapturedRaggedBatchForward``, ``CapturedTrainStep``, ``CapturedRaggedBatchStep``, ``train`` / ``evaluate`` / ``predict``) against the
eager SIZED model on the same weights.

Models and inputs are those of tests/test_gpu_topk_pool_model.py (seed 4, ``SHARPEN``) and the seeds of
tests/option_crossing_cases.py: the conditions asserted on them in tests/test_topk_pool_host.py and
tests/test_option_crossings_host.py are properties of the weights and inputs, which the padded form does not change.  Bars: logits
and loss 1e-5, gradients ``2e-5 + 1e-4 max|ref|`` per tensor."""
import numpy as np
import pytest
import torch

from oracle import graphnet_oracle as O
from tests import option_crossing_cases as X
from tests import topk_pool_cases as K
from tests import test_gpu_topk_pool_model as M
from tests._util import max_abs
from tests.capture_lifetime_cases import replay_between_allocations
from tests.test_gpu_attention_readout_model import SIX, THREE, _graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO, READOUTS = M.RATIO, M.READOUTS


def _padded(readout="mean", **extra):
    return M._model(readout, pool_padded=True, **extra)


def _dev(sample):
    return tuple(t.to(DEV) for t in sample)


def _sized_twin(m, readout="mean", **extra):
    """The eager SIZED model on the weights of ``m`` (same keys: ``pool_padded`` adds none)."""
    twin = M._model(readout, **extra)
    twin.load_state_dict(m.state_dict())
    return twin


@pytest.fixture(scope="module")
def inputs():
    return M._inputs()


def test_the_model_is_padded_and_has_the_sized_models_weights():
    from graphnet_classifier_amd.GNN import pooling_reads_sizes_back, uses_node_pooling
    m, s = _padded("mean"), M._model("mean")
    assert m.graph_net.pool_padded and all(p.padded for p in m.graph_net.graph_processor.pools.values())
    assert uses_node_pooling(m) and not pooling_reads_sizes_back(m) and pooling_reads_sizes_back(s)
    assert list(m.state_dict()) == list(s.state_dict()) and all(torch.equal(v, s.state_dict()[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("readout", READOUTS)
def test_logits_and_kept_nodes_match_the_composed_oracle(inputs, readout):
    m = _padded(readout).eval()
    sd = M._sd(m)
    singles = []
    for name, x, pos, ei, gp in inputs:
        ref, kept_ref = K.pooled_logits(sd, x, pos, ei, RATIO, (0, 1), readout, gp)
        with torch.no_grad():
            if gp is None:
                logits = m(_dev((x, pos, ei))).cpu()[None]
                kept = m.kept_nodes(*_dev((x, pos, ei)))
                assert kept.dtype == torch.int64 and kept.is_cuda and not kept.requires_grad
                assert np.array_equal(kept.cpu().numpy(), kept_ref) and kept.numel() == m.graph_net.pooled_nodes(x.size(0))
                singles.append(logits[0])
            else:
                logits = m.forward_batched(*_dev((x, pos, ei)), graph_ptr=torch.tensor(gp)).cpu()
        print(f"padded, {readout}, {name}: |device - oracle| = {max_abs(logits, ref):.3e}")
        assert logits.shape == ref.shape and max_abs(logits, ref) <= 1e-5
    b = M._batch([c for c, _ in THREE])
    with torch.no_grad():
        batched = m.forward_batched(b.x.to(DEV), b.pos.to(DEV), b.edge_index.to(DEV), graph_ptr=b.graph_ptr).cpu()
    assert batched.shape == (3, 2) and max_abs(batched, torch.stack(singles)) <= 1e-5


def test_forward_device_keeps_every_row_and_the_public_forward_narrows(inputs):
    """``forward_device(return_pooling=True)``: ``out`` [rows, out_dim], ``graph_ptr'`` that ends at N', ``kept`` [rows] with -1 behind
    N' and the composed survivors in front (a -1 of the second layer must not index the first layer's list).  ``GraphNet.forward``
    narrows to N' and equals the sized model's rows within the bar."""
    from graphnet_classifier_amd.topology import get_topology
    m = _padded("mean").eval()
    sized = _sized_twin(m).eval()
    _, x, pos, ei, _ = inputs[0]
    xd, pd, ed = _dev((x, pos, ei))
    _, kept_ref = K.pooled_logits(M._sd(m), x, pos, ei, RATIO, (0, 1), "mean")
    with torch.no_grad():
        out, gp, kept = m.graph_net.forward_device(xd, pd, get_topology(ed, x.size(0), DEV), return_pooling=True)
        public, want = m.graph_net(xd, pd, ed), sized.graph_net(xd, pd, ed)
    n_out = m.graph_net.pooled_nodes(x.size(0))
    assert out.shape == (x.size(0), M.OUT_DIM) and gp.tolist() == [0, n_out] and kept.shape == (x.size(0),) and kept.dtype == torch.int32
    assert np.array_equal(kept[:n_out].cpu().numpy(), kept_ref) and bool((kept[n_out:] == -1).all())
    assert public.shape == want.shape == (n_out, M.OUT_DIM) and max_abs(public, want) <= 1e-5 and max_abs(out[:n_out], want) <= 1e-5
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("readout", READOUTS)
def test_gradients_against_float64_autograd(readout):
    x, pos, ei = _graph(20)
    label = torch.tensor(1)
    m = _padded(readout)
    torch.nn.CrossEntropyLoss()(m(_dev((x, pos, ei))), label.to(DEV)).backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    O.set_scatter_impl("index_add")  # the differentiable ATen form of the same sum
    try:
        logits, _ = K.pooled_logits(sd, x.double(), pos.double(), ei, RATIO, (0, 1), readout)
    finally:
        O.set_scatter_impl("sorted_loop")
    torch.nn.functional.cross_entropy(logits, label[None]).backward()
    ref = {k: v.grad for k, v in sd.items()}
    scorers = [k for k in got if ".pools." in k]
    assert len(scorers) == 8 and set(ref) == set(got)
    for k in scorers:
        assert bool(got[k].any()) and bool(ref[k].any()), k
    M._assert_gradients(got, ref, f"eager padded step, readout={readout}")


def test_a_pooled_graph_without_edges_runs_the_remaining_blocks():
    """The edge-less case of tests/test_gpu_topk_pool_model.py in padded form: behind the first layer E' = 0, so all 90 edge slots
    are slack self-loops of the 20 slack rows, and block 2 runs on them."""
    _, x, pos, ei = X.edgeless_case("sum")  # (its model is the sized one: the padded one below gets the same scorers)
    m = _padded("mean").eval()
    with torch.no_grad():
        for pool in m.graph_net.graph_processor.pools.values():
            pool.gate.model[2].weight.zero_()
            pool.gate.model[2].bias.fill_(0.7)
    ref, kept_ref = K.pooled_logits(M._sd(m), x, pos, ei, RATIO, (0, 1), "mean")
    assert kept_ref.tolist() == list(range(10))
    with torch.no_grad():
        logits = m(_dev((x, pos, ei))).cpu()
        kept = m.kept_nodes(*_dev((x, pos, ei)))
    assert kept.tolist() == list(range(10)) and max_abs(logits, ref[0]) <= 1e-5
    m.train()
    m(_dev((x, pos, ei))).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


@pytest.mark.parametrize("crossing", [c for c in X.FORWARD_ROWS if c.readout == "mean"], ids=lambda c: c.id)
def test_crossings_on_the_batch_of_six(inputs, crossing):
    c = crossing
    m = _padded(c.readout, seed=c.seed, aggregation=c.aggregation).eval()
    name, x, pos, ei, gp = inputs[3]
    ref, _ = X.crossed_logits(c.aggregation, X.state(m), x, pos, ei, RATIO, X.POOL_AFTER, c.readout, gp)
    with torch.no_grad():
        logits = m.forward_batched(*_dev((x, pos, ei)), graph_ptr=torch.tensor(gp)).cpu()
    print(f"padded, {c.id}, {name}: |device - oracle| = {max_abs(logits, ref):.3e}")
    assert logits.shape == ref.shape and max_abs(logits, ref) <= 1e-5


@pytest.mark.parametrize("readout", READOUTS)
def test_unpooled_fixed_topology_replays_survive_later_allocations(readout):
    """The same buffer serves the pooled read-out of a model WITHOUT pooling layers (``readout_logits(y, [0, N])``)."""
    from graphnet_classifier_amd.GNN import CapturedForward
    m = M._model(readout, pool_ratio=None).eval()
    sample, other = _dev(_graph(THREE[0][0])), _dev(_graph(THREE[1][0]))
    with torch.no_grad():
        want = m(sample)
    replay_between_allocations(CapturedForward(m, *sample), sample, want, m, other, f"un-pooled, {readout}")


@pytest.mark.parametrize("readout", READOUTS)
def test_captured_forwards_equal_the_eager_sized_model(readout):
    from graphnet_classifier_amd.GNN import CapturedForward, CapturedRaggedBatchForward
    m = _padded(readout).eval()
    sized = _sized_twin(m, readout).eval()
    on_dev = {c: _dev(_graph(c)) for c, _ in THREE}
    with torch.no_grad():
        want = {c: sized(on_dev[c]) for c in on_dev}
    first = THREE[0][0]
    fixed = CapturedForward(m, *on_dev[first])  # one fixed topology
    replay_between_allocations(fixed, on_dev[first], want[first], sized, on_dev[THREE[1][0]], f"padded, {readout}")
    any_topology = CapturedForward(m, *on_dev[first], edge_capacity=1024)  # any edge list over the 69 nodes
    assert max_abs(any_topology(*on_dev[first]), want[first]) <= 1e-5
    any_topology.check()
    ragged = CapturedForward(m, *on_dev[first], edge_capacity=1024, node_capacity=128)  # 69 / 119 / 100 nodes
    for c, nodes in THREE:
        got = ragged(*on_dev[c])
        print(f"padded, {readout}, captured over a node capacity, {nodes} nodes: |captured - eager sized| = {max_abs(got, want[c]):.3e}")
        assert max_abs(got, want[c]) <= 1e-5, nodes
    ragged.check()
    batches = [M._batch(SIX[:3]), M._batch(SIX[3:])]
    cap = CapturedRaggedBatchForward(m, batches[0].to(DEV), edge_capacity=2048, node_capacity=512)
    for b in reversed(batches):
        with torch.no_grad():
            eager = sized.forward_batched(b.x.to(DEV), b.pos.to(DEV), b.edge_index.to(DEV), graph_ptr=b.graph_ptr)
        assert cap.matches(b) and max_abs(cap(b.to(DEV)), eager) <= 1e-5
    cap.check()


def _eager_sized_loss_and_gradients(state_dict, forward, label):
    """Loss and gradients of ONE eager step of the SIZED model from the given parameters."""
    e = M._model("mean")
    e.load_state_dict(state_dict)
    loss = torch.nn.CrossEntropyLoss()(forward(e), label.to(DEV))
    loss.backward()
    return float(loss.item()), {k: p.grad.clone() for k, p in e.named_parameters()}


def test_captured_train_step_over_a_node_capacity_equals_eager_sized_steps():
    from graphnet_classifier_amd.train import CapturedTrainStep, FlatParameters, FusedAdam
    crit = torch.nn.CrossEntropyLoss()
    m = _padded("mean")
    opt = FusedAdam(FlatParameters(m))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = CapturedTrainStep(m, opt, crit, _graph(THREE[1][0]), torch.tensor(0), loss_sum, edge_capacity=1024, node_capacity=128)
    torch.cuda.synchronize()
    assert float(loss_sum.item()) == 0.0 and all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    seen = 0.0
    for (case_id, nodes), label in zip(THREE, (torch.tensor(1), torch.tensor(0), torch.tensor(1))):
        sample = _graph(case_id)
        start = {k: v.detach().clone() for k, v in m.state_dict().items()}
        loss, want = _eager_sized_loss_and_gradients(start, lambda e: e(_dev(sample)), label)
        assert step.matches(sample)
        step(sample, label)
        step.check()
        torch.cuda.synchronize()
        total = float(loss_sum.item())
        print(f"padded, {nodes} nodes: captured loss {total - seen:.8f}, eager sized {loss:.8f}")
        assert abs((total - seen) - loss) <= 1e-5
        seen = total
        M._assert_gradients(dict(zip(opt.fp.names, opt.fp.reducer.views)), want, f"captured padded step on {nodes} nodes")
        assert any(not torch.equal(start[k], v) for k, v in m.state_dict().items())


def test_captured_ragged_batch_step_equals_eager_sized_steps():
    from graphnet_classifier_amd.train import CapturedRaggedBatchStep, FlatParameters, FusedAdam, padded_capacity
    crit = torch.nn.CrossEntropyLoss()
    batches = [M._batch(SIX[:3]), M._batch(SIX[3:])]
    labels = [torch.tensor([0, 1, 1]), torch.tensor([1, 0, 1])]
    E = padded_capacity(max(b.num_edges for b in batches))
    N = padded_capacity(max(b.num_nodes for b in batches), 0, 32)
    m = _padded("mean")
    opt = FusedAdam(FlatParameters(m))
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    step = CapturedRaggedBatchStep(m, opt, crit, batches[0].to(DEV), labels[0], loss_sum, edge_capacity=E, node_capacity=N)
    torch.cuda.synchronize()
    assert float(loss_sum.item()) == 0.0 and int(opt.step_count.item()) == 0
    seen = 0.0
    for b, lab in zip(reversed(batches), reversed(labels)):  # the other batch first
        start = {k: v.detach().clone() for k, v in m.state_dict().items()}
        loss, want = _eager_sized_loss_and_gradients(
            start, lambda e: e.forward_batched(b.x.to(DEV), b.pos.to(DEV), b.edge_index.to(DEV), graph_ptr=b.graph_ptr), lab)
        step(b.to(DEV), lab)
        step.check()
        torch.cuda.synchronize()
        total = float(loss_sum.item())
        print(f"padded, {b.num_nodes} nodes: captured loss {total - seen:.8f}, eager sized {loss:.8f}")
        assert abs((total - seen) - loss) <= 1e-5
        seen = total
        M._assert_gradients(dict(zip(opt.fp.names, opt.fp.reducer.views)), want, f"captured padded batch step on {b.num_nodes} nodes")
    assert int(opt.step_count.item()) == 2


def test_an_edge_id_outside_the_graph_gives_nan_and_check_raises():
    from graphnet_classifier_amd.GNN import CapturedForward
    m = _padded("mean").eval()
    x, pos, ei = _dev(_graph(THREE[0][0]))
    cap = CapturedForward(m, x, pos, ei, edge_capacity=1024)
    assert bool(torch.isfinite(cap(x, pos, ei)).all())
    cap.check()
    bad = ei.clone()
    bad[0, 3] = 100000  # outside the padded buffers as well: the topology build's own flag
    assert bool(torch.isnan(cap(x, pos, bad)).all())
    with pytest.raises(IndexError):
        cap.check()
    assert bool(torch.isfinite(cap(x, pos, ei)).all())  # and the capture serves the next good sample
    cap.check()


def test_train_evaluate_and_predict_capture_a_padded_model(tmp_path):
    from graphnet_classifier_amd.train import evaluate, predict, train
    m = _padded("mean")
    sample = _graph(35)
    dataset = [(sample, torch.tensor(k % 2)) for k in range(4)]  # one topology four times
    history = train(m, dataset, epochs=2, output_path=str(tmp_path), capture=True)
    assert len(history["avg_loss"]) == 2 and all(np.isfinite(v) for v in history["avg_loss"])
    assert history["captured"] is True
    loader = [(M._batch([a, b]), torch.tensor([k % 2, (k + 1) % 2])) for k, (a, b) in enumerate(zip(SIX[0::2], SIX[1::2]))]
    m.eval()
    ev_c, ev_e = evaluate(m, loader, capture=True), evaluate(m, loader, capture=False)
    assert ev_c["count"] == ev_e["count"] == 6 and torch.equal(ev_c["confusion"], ev_e["confusion"])
    assert abs(ev_c["loss"] - ev_e["loss"]) <= 1e-5
    (logits_c, prob_c), (logits_e, prob_e) = predict(m, loader, capture=True), predict(m, loader, capture=False)
    print(f"padded predict: max |captured - eager| = {max_abs(logits_c, logits_e):.3e}")
    assert logits_c.shape == logits_e.shape == (6, 2) and max_abs(logits_c, logits_e) <= 1e-5 and max_abs(prob_c, prob_e) <= 1e-5
    # the ragged mini-batches were replayed, not run eagerly: the scorer of evaluate / predict holds a capture after three batches
    from graphnet_classifier_amd.train import _BatchScorer
    score = _BatchScorer(m, torch.device(DEV), True)
    assert score.capture
    with torch.no_grad():
        for batch, _ in loader:
            score(batch)
    assert score.ragged.current is not None


def test_what_stays_refused():
    """A sized pooled model is refused by every capture as before (tests/test_gpu_topk_pool_model.py holds the full list); a padded
    model under the flatten read-out, and a bare padded GraphNet, keep the ValueError that names pooling."""
    from graphnet_classifier_amd.GNN import CapturedForward, CombinedModel
    from graphnet_classifier_amd.train import CapturedTrainStep, FlatParameters, FusedAdam
    sample = _dev(_graph(35))
    crit = torch.nn.CrossEntropyLoss()
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    sized = M._model("mean")
    with pytest.raises(ValueError, match="pooling"):
        CapturedForward(sized, *sample, edge_capacity=1024)
    with pytest.raises(ValueError, match="pooling"):
        CapturedTrainStep(sized, FusedAdam(FlatParameters(sized)), crit, sample, torch.tensor(0), loss_sum)
    padded = _padded("mean")
    with pytest.raises(ValueError, match="pooling"):
        CapturedForward(padded.graph_net, *sample)
    flat = CombinedModel(padded.graph_net, num_nodes=padded.graph_net.pooled_nodes(100), classes=2)
    with pytest.raises(ValueError, match="pooling"):
        CapturedForward(flat, *sample)
    with pytest.raises(ValueError, match="pooling"):
        CapturedTrainStep(flat, FusedAdam(FlatParameters(flat)), crit, sample, torch.tensor(0), loss_sum)
    # eagerly the flatten read-out works on the narrowed rows, as the sized model's does
    with torch.no_grad():
        sized_flat = CombinedModel(sized.graph_net, num_nodes=flat.num_nodes, classes=2)
        sized_flat.load_state_dict(flat.state_dict())
        assert max_abs(flat.eval()(sample), sized_flat.eval()(sample)) <= 1e-5
