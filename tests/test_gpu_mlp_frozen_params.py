"""GPU: the fused-MLP backward with a subset of the parameters frozen.  A frozen parameter gets no gradient and every other
parameter gets, bit for bit, the gradient of the all-trainable run of the same model on the same input: freezing a parameter
leaves out products of the weight-gradient assembly, it never changes the data kernel (every MLP's input still wants its
gradient) nor the products that remain.  Widths 64 (the fused K8 kernel hands out dw / db itself; the node processors take the
split path with two first-layer blocks) and 128 (every MLP on the split path), a batch below and one above the row limits of
the small-batch forward and of the one-launch weight gradients; the layer-by-layer backward (Tanh) and the wide first Linear."""
import functools

import pytest
import torch
from torch import nn

from graphnet_classifier_amd import functional as Fn
from graphnet_classifier_amd import native
from graphnet_classifier_amd import synthetic as S
from tests import image_mlp_cases as C
from tests._util import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS, BATCHES = (64, 128), (6, 42)  # superpixel_like_graphs(6 | 42, seed=11): 925 nodes / 4,966 edges and 6,640 / 35,700


def _freeze_weights(model):
    return [p for n, p in model.named_parameters() if n.endswith(".weight")]


def _freeze_layernorms(model):
    return [p for m in model.modules() if isinstance(m, nn.LayerNorm) for p in m.parameters()]


def _freeze_edge_first_weight(model):
    from graphnet_classifier_amd.GNN import EdgeProcessor
    return [m.edge_processor.model[0].weight for m in model.modules() if isinstance(m, EdgeProcessor)]


def _freeze_block0_edge_model(model):
    return list(model.graph_processor.blocks[0].edge_model.parameters())


PATTERNS = {"weights": _freeze_weights, "layernorms": _freeze_layernorms, "edge_first_weight": _freeze_edge_first_weight,
            "block0_edge_model": _freeze_block0_edge_model}


@functools.lru_cache(maxsize=None)
def _inputs(num_graphs):
    batch = S.superpixel_like_graphs(num_graphs, seed=11)
    torch.manual_seed(3)
    return batch.x.to(DEV), batch.pos.to(DEV), batch.edge_index.to(DEV), torch.randn(batch.num_nodes, 1, device=DEV)


def _model(width, activation="ReLU"):
    from graphnet_classifier_amd.GNN import GraphNet
    torch.manual_seed(5)
    return GraphNet(**S.graphnet_kwargs(width, 2), activation=activation)


def _backward(model, num_graphs, x=None):
    x0, pos, ei, w = _inputs(num_graphs)
    (model(x0 if x is None else x, pos, ei) * w).sum().backward()
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}


@functools.lru_cache(maxsize=None)
def _all_trainable(width, num_graphs, activation="ReLU"):
    return _backward(_model(width, activation), num_graphs)


def _assert_frozen_run_equals_all_trainable(model, frozen, got, want):
    frozen = {id(p) for p in frozen}
    assert frozen
    for k, p in model.named_parameters():
        if id(p) in frozen:
            assert got[k] is None, k
        else:
            assert want[k] is not None and got[k] is not None and torch.equal(got[k], want[k]), k


def test_batches_lie_on_both_sides_of_the_row_limits():
    lib = native.load_library()
    limits = (int(lib.gnc_mlp_small_batch_max_rows()), int(lib.gnc_xty_small_max_rows()))
    small, large = (_inputs(g)[2].size(1) for g in BATCHES)
    assert all(small <= lim < large for lim in limits), (small, large, limits)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("num_graphs", BATCHES)
@pytest.mark.parametrize("width", WIDTHS)
def test_frozen_pattern_leaves_the_other_gradients_bit_equal(width, num_graphs, pattern):
    want = _all_trainable(width, num_graphs)
    model = _model(width)
    frozen = PATTERNS[pattern](model)
    for p in frozen:
        p.requires_grad_(False)
    _assert_frozen_run_equals_all_trainable(model, frozen, _backward(model, num_graphs), want)


@pytest.mark.parametrize("num_graphs", BATCHES)
@pytest.mark.parametrize("width", WIDTHS)
def test_inputs_only_gradient_agrees_with_torch_recompute(width, num_graphs, monkeypatch):
    """Every parameter frozen, x wants its gradient: against the PyTorch-ROCm recompute backward (HIP_BACKWARD = False) at the
    two bounds of test_gpu_model.test_hip_backward_agrees_with_torch_recompute_backward."""
    model = _model(width)
    for p in model.parameters():
        p.requires_grad_(False)
    dx = {}
    for hip in (True, False):
        monkeypatch.setattr(Fn, "HIP_BACKWARD", hip)
        x = _inputs(num_graphs)[0].clone().requires_grad_(True)
        grads = _backward(model, num_graphs, x)
        assert all(g is None for g in grads.values())
        dx[hip] = x.grad
    a, b = dx[True], dx[False]
    assert bool(torch.isfinite(a).all())
    rel, worst = float((a - b).norm() / b.norm().clamp_min(1e-12)), max_abs(a, b)
    print(f"width {width}, {num_graphs} graphs: dx rel {rel:.2e}, max abs {worst:.2e} of {float(b.abs().max()):.2e}")
    assert rel < 1e-3
    assert worst < 3e-3 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("pattern", ["weights", "layernorms"])
def test_frozen_pattern_through_the_layerwise_backward(pattern, monkeypatch):
    """activation="Tanh": every MLP's backward runs layer by layer (functional._layerwise_mlp_backward_hip)."""
    calls = []
    real = Fn._layerwise_mlp_backward_hip
    monkeypatch.setattr(Fn, "_layerwise_mlp_backward_hip", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    want = _all_trainable(64, BATCHES[0], "Tanh")
    model = _model(64, "Tanh")
    frozen = PATTERNS[pattern](model)
    for p in frozen:
        p.requires_grad_(False)
    before = len(calls)
    got = _backward(model, BATCHES[0])
    assert len(calls) > before
    _assert_frozen_run_equals_all_trainable(model, frozen, got, want)


@pytest.mark.parametrize("frozen_name", ["model.0.weight", "model.0.bias"])
def test_wide_first_linear_with_one_of_its_parameters_frozen(frozen_name, monkeypatch):
    """_WideFirstMLP (8 rows, a first Linear of 1200 inputs): W0 frozen with b0 trainable, and the reverse."""
    monkeypatch.delenv("GNC_NO_WIDE_LINEAR", raising=False)
    case = (8, 1200, 128, 2)
    x, g = C.inputs(case).to(DEV), C.cotangent(case).to(DEV)
    grads = {}
    for frozen in (None, frozen_name):
        model = C.reference_mlp(case, "ReLU", "LayerNorm")
        lin = [m for m in model.model if isinstance(m, nn.Linear)]
        assert Fn.wide_linear_route([(x, None)], [m.weight for m in lin], [m.bias for m in lin], None, "ReLU", None, None)
        if frozen is not None:
            dict(model.named_parameters())[frozen].requires_grad_(False)
        model(x).backward(g)
        grads[frozen] = {k: p.grad for k, p in model.named_parameters()}
    for k, want in grads[None].items():
        got = grads[frozen_name][k]
        if k == frozen_name:
            assert got is None
        else:
            assert want is not None and torch.equal(got, want), k
