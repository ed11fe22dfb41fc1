"""GPU: the batched read-out (csrc/readout_batched.hip, ``functional.readout_batched``) against the float64 oracle per graph -
logits, all six parameter gradients and ``dy`` at ``|d| <= 1e-5 * max(1, max|ref|)`` -, its exact zeros, run-to-run equality,
NaN containment, and ``CombinedModel.forward_batched`` on top of it in both modes.  Cases, seeds and references:
tests/readout_batched_cases.py (no graph is excused for a ReLU near zero: the seeds keep every float64 pre-activation at least
1e-5 away from it, asserted on the host in tests/test_minibatch_host.py)."""
import pytest
import torch

from oracle import graphnet_oracle as O
from tests import readout_batched_cases as R
from tests._util import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
NAMES = [c.name for c in R.CASES]


def _bound(ref):
    return TOL * max(1.0, float(ref.abs().max()))


def _device_inputs(ref):
    c = ref["case"]
    y = ref["y"].to(DEV).requires_grad_(True)
    params = [ref["sd"][f"classifier.{n}.{p}"].to(DEV).requires_grad_(True) for n in ("fc1", "fc2", "fc3") for p in ("weight", "bias")]
    gp = ref["graph_ptr"].to(DEV) if c.use_graph_ptr else None
    return c, y, params, gp


def _run(ref, backward=True):
    from graphnet_classifier_amd import functional as Fn
    c, y, params, gp = _device_inputs(ref)
    logits = Fn.readout_batched(y, gp, c.num_graphs, c.num_nodes, *params)
    if not backward:
        return logits.detach(), None
    poison = torch.full((y.numel() + 64,), float("nan"), device=DEV)  # what torch.empty hands the backward next: not zeros
    del poison
    logits.backward(ref["grad_logits"].to(DEV))
    return logits.detach(), (y.grad,) + tuple(p.grad for p in params)


@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_the_float64_oracle(name):
    ref = R.build(name)
    logits, _ = _run(ref, backward=False)
    err = max_abs(logits.cpu(), ref["logits"])
    print(f"{name}: |logits - oracle| = {err:.3e} (bound {_bound(ref['logits']):.1e})")
    assert logits.shape == ref["logits"].shape and err <= _bound(ref["logits"])


@pytest.mark.parametrize("name", NAMES)
def test_backward_matches_float64_autograd(name):
    ref = R.build(name)
    _, grads = _run(ref)
    errs = {n: (max_abs(g.cpu(), r), _bound(r)) for n, g, r in zip(ref["grad_names"], grads, ref["grads"])}
    print(name + ": " + ", ".join(f"{n} {e:.2e}/{b:.1e}" for n, (e, b) in errs.items()))
    for n, g, r in zip(ref["grad_names"], grads, ref["grads"]):
        assert g.shape == r.shape, n
    assert all(e <= b for e, b in errs.values()), errs


@pytest.mark.parametrize("name", ["smaller_equal_larger", "two_tiles_plus_one_odd_F", "several_F_slices", "tail_tiles"])
def test_two_runs_are_bitwise_equal(name):
    ref = R.build(name)
    l1, g1 = _run(ref)
    l2, g2 = _run(ref)
    assert torch.equal(l1, l2)
    for a, b, n in zip(g1, g2, ref["grad_names"]):
        assert torch.equal(a, b), n


def test_num_graphs_and_uniform_graph_ptr_agree_bit_for_bit():
    a, b = R.build("equal_via_num_graphs"), R.build("equal_via_graph_ptr")
    assert torch.equal(a["y"], b["y"]) and not a["case"].use_graph_ptr and b["case"].use_graph_ptr
    la, ga = _run(a)
    lb, gb = _run(b)
    assert torch.equal(la, lb)
    for x, y, n in zip(ga, gb, a["grad_names"]):
        assert torch.equal(x, y), n


def test_the_query_reports_more_than_one_slice_of_F():
    from graphnet_classifier_amd import native
    c = R.BY_NAME["several_F_slices"]
    plan = native.readout_batched_plan(c.num_graphs, c.features, R.H1, R.H2, c.classes)
    assert plan is not None and plan["f_slices"] > 1 and plan["f_slices"] * plan["f_slice_len"] >= c.features
    assert plan["forward_workspace_floats"] == plan["f_slices"] * c.num_graphs * R.H1
    c = R.BY_NAME["tail_tiles"]
    plan = native.readout_batched_plan(c.num_graphs, c.features, R.H1, R.H2, c.classes)
    assert plan["tail_rows"] == 16 and plan["dw1_parts"] > 1 and plan["small_parts"] > 1


def test_dy_rows_behind_num_nodes_are_exact_zeros():
    ref = R.build("smaller_equal_larger")
    c = ref["case"]
    _, grads = _run(ref)
    dy, start = grads[0], 0
    checked = 0
    for size in c.sizes:
        if size > c.num_nodes:
            tail = dy[start + c.num_nodes:start + size]
            assert tail.numel() and torch.equal(tail, torch.zeros_like(tail))
            checked += 1
        start += size
    assert checked == 1 and not torch.isnan(dy).any()


def test_dw1_columns_no_graph_reaches_are_exact_zeros():
    from graphnet_classifier_amd import functional as Fn
    torch.manual_seed(7)
    num_nodes, sizes = 156, (144,) * 4
    y = torch.randn(sum(sizes), 1, device=DEV)
    fc = [torch.nn.Linear(num_nodes, R.H1), torch.nn.Linear(R.H1, R.H2), torch.nn.Linear(R.H2, 2)]
    params = [p.detach().to(DEV).requires_grad_(True) for m in fc for p in (m.weight, m.bias)]
    gp = torch.tensor([0, 144, 288, 432, 576], device=DEV)
    poison = torch.full((R.H1 * num_nodes + 64,), float("nan"), device=DEV)
    del poison
    Fn.readout_batched(y, gp, 4, num_nodes, *params).backward(torch.randn(4, 2, device=DEV))
    dw1 = params[0].grad
    assert torch.equal(dw1[:, 144:], torch.zeros_like(dw1[:, 144:])) and dw1[:, :144].abs().max() > 0


def test_a_nan_row_poisons_its_own_graph_only():
    from graphnet_classifier_amd import functional as Fn
    ref = R.build("smaller_equal_larger")
    c, y, params, gp = _device_inputs(ref)
    clean = Fn.readout_batched(y.detach(), gp, c.num_graphs, c.num_nodes, *[p.detach() for p in params])
    bad = y.detach().clone()
    bad[int(ref["graph_ptr"][1]) + 3] = float("nan")  # a row of graph 1
    out = Fn.readout_batched(bad, gp, c.num_graphs, c.num_nodes, *[p.detach() for p in params])
    assert torch.isnan(out[1]).all()
    keep = [0, 2, 3, 4]
    assert torch.equal(out[keep], clean[keep])


# ------------------------------------------------------------------------------------------------ model level
def _model_and_batch(equal: bool):
    from graphnet_classifier_amd import synthetic
    from graphnet_classifier_amd.GNN import CombinedModel, GraphNet
    shapes = ((12, 13),) if equal else ((12, 12), (12, 13), (13, 13))
    batch = synthetic.superpixel_like_graphs(5, seed=1000, shapes=shapes)
    torch.manual_seed(11)
    model = CombinedModel(GraphNet(**synthetic.graphnet_kwargs(32, 1)), num_nodes=156, classes=2)
    return model, batch


def _oracle_logits(sd, batch, num_nodes):
    out = []
    for g in range(batch.num_graphs):
        b = batch.slice_graphs(g, g + 1)
        y = O.graphnet_forward(sd, b.x, b.pos, b.edge_index, prefix="graph_net.")
        out.append(O.classifier_forward(sd, R.gather_features(y, torch.tensor([0, y.size(0)]), num_nodes)[0]))
    return torch.stack(out)


@pytest.mark.parametrize("equal", [True, False], ids=["num_graphs", "graph_ptr"])
def test_forward_batched_runs_the_kernel_and_matches_the_oracle(equal, monkeypatch):
    from graphnet_classifier_amd import GNN, native
    model, batch = _model_and_batch(equal)
    if not equal:
        assert len(set((batch.graph_ptr[1:] - batch.graph_ptr[:-1]).tolist())) > 1
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = _oracle_logits(sd, batch, 156)
    args = (batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV))
    kw = dict(num_graphs=5) if equal else dict(graph_ptr=batch.graph_ptr)
    timers = native.KernelTimers()
    native.set_kernel_timers(timers)
    try:
        with torch.no_grad():
            logits = model.forward_batched(*args, **kw)
        torch.cuda.synchronize()
    finally:
        native.set_kernel_timers(None)
    assert "readout_batched_forward" in timers.events, sorted(timers.events)
    monkeypatch.setattr(GNN, "READOUT_HIP", False)
    with torch.no_grad():
        torch_path = model.forward_batched(*args, **kw)
    print(f"|kernel - oracle| = {max_abs(logits.cpu(), ref):.3e}, |kernel - torch path| = {max_abs(logits, torch_path):.3e}")
    assert logits.shape == (5, 2)
    assert max_abs(logits.cpu(), ref) <= TOL and max_abs(logits, torch_path) <= TOL


def test_forward_batched_gradients_match_the_torch_path(monkeypatch):
    """The kernel path's parameter gradients against the torch path's (same GraphNet backward under both), ragged batch."""
    from graphnet_classifier_amd import GNN
    model, batch = _model_and_batch(False)
    args = (batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV))
    labels = torch.tensor([0, 1, 1, 0, 1], device=DEV)

    def grads():
        model.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model.forward_batched(*args, graph_ptr=batch.graph_ptr), labels).backward()
        return {n: p.grad.clone() for n, p in model.named_parameters()}
    hip = grads()
    monkeypatch.setattr(GNN, "READOUT_HIP", False)
    ref = grads()
    worst = max((max_abs(hip[n], ref[n]) / max(1.0, float(ref[n].abs().max())), n) for n in ref)
    print(f"worst relative gradient difference {worst[0]:.3e} at {worst[1]}")
    assert worst[0] <= TOL
