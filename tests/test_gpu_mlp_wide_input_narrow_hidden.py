"""GPU: the fused-MLP backward for an input wider than every later layer - ``MLP(64, 1, hidden_dim=32)``, the shape of the top-K
pooling scorer (K20) under a 64-wide GraphNet.  The weights-resident data kernel forms a segment's input gradient in tiles of 32
columns and used to take their number from the hidden and output widths alone, so columns 32..63 of ``dx`` were never formed.  Every
gradient against float64 autograd of the same MLP, at the bar of the other gradient tests (2e-5 + 1e-4 max|reference|)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("shape", ((64, 32, 1), (48, 32, 1), (64, 16, 8), (40, 8, 4), (64, 64, 1), (8, 32, 1)))
@pytest.mark.parametrize("rows", (35, 300))
def test_input_and_weight_gradients(shape, rows):
    from graphnet_classifier_amd.MLP import MLP
    C, H, out = shape
    torch.manual_seed(C + H + out)
    mlp = MLP(C, out, hidden_dim=H, hidden_layers=1, activation="ReLU", norm_type=None).to(DEV)
    x0, v = torch.randn(rows, C), torch.randn(rows, out)
    v[::2] = 0.0  # rows with an exact zero gradient, as behind a pooling layer
    x = x0.to(DEV).requires_grad_(True)
    (mlp.forward_segments([(x, None)]) * v.to(DEV)).sum().backward()
    sd = {k: p.detach().cpu().double().requires_grad_(True) for k, p in mlp.state_dict().items()}
    x64 = x0.double().requires_grad_(True)
    y64 = torch.relu(x64 @ sd["model.0.weight"].t() + sd["model.0.bias"]) @ sd["model.2.weight"].t() + sd["model.2.bias"]
    (y64 * v.double()).sum().backward()
    got = {"x": x.grad, **{k: p.grad for k, p in mlp.named_parameters()}}
    ref = {"x": x64.grad, **{k: p.grad for k, p in sd.items()}}
    for k, r in ref.items():
        err = float((got[k].cpu().double() - r).abs().max())
        assert err <= 2e-5 + 1e-4 * float(r.abs().max()), f"{shape} x {rows} rows: {k} err {err:.3e}"
