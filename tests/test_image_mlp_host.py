"""Host side of the image-MLP baseline (no GPU): the float64 formulas of tests/image_mlp_cases.py against torch.nn, the ReLU
margin of every case, the golden captured from the reference's MLP and train(), the loader's index batches against
torch.utils.data.DataLoader, the new C-ABI symbols, and the host-side decision of K16 (gnc_wide_linear_supported)."""
import os
import re

import numpy as np
import pytest
import torch

from graphnet_classifier_amd import dataset as D
from graphnet_classifier_amd import native
from tests import image_mlp_cases as C
from tests._util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gnc_wide_linear_supported", "gnc_wide_linear_workspace_floats", "gnc_wide_linear_forward_f32",
               "gnc_wide_linear_backward_f32", "gnc_u8_hwc_to_f32_chw")


# ---------------------------------------------------------------- formulas against torch.nn in float64
@pytest.mark.parametrize("case", [(5, 1083, 40, 2), (16, 1200, 64, 5)], ids=C.case_id)
@pytest.mark.parametrize("activation", ["ReLU", "GELU", "Identity"])
@pytest.mark.parametrize("norm_type", ["LayerNorm", None])
def test_formulas_equal_torch_nn_float64(case, activation, norm_type):
    model = C.reference_mlp(case, activation, norm_type).cpu().double()
    w, b, gamma, beta, eps = C.params64(model)
    x, g = C.inputs(case), C.cotangent(case)
    out, *_ = C.forward64(x, w, b, gamma, beta, eps, activation)
    want = model.model(x.double())
    assert float((out - want.detach()).abs().max()) < 1e-12
    want.backward(g.double())
    grads = C.backward64(x, w, b, gamma, beta, eps, g, activation)
    lin = [m for m in model.model if isinstance(m, torch.nn.Linear)]
    for k, m in enumerate(lin):
        scale = max(1.0, float(m.weight.grad.abs().max()))
        assert float((grads["w"][k] - m.weight.grad).abs().max()) < 1e-12 * scale
        assert float((grads["b"][k] - m.bias.grad).abs().max()) < 1e-12 * scale
    if norm_type is not None:
        assert float((grads["gamma"] - model.model[-1].weight.grad).abs().max()) < 1e-12
        assert float((grads["beta"] - model.model[-1].bias.grad).abs().max()) < 1e-12


def test_to_tensor_formula_is_permute_float_div():
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3)[:5 * 7 * 3].reshape(5, 7, 3)
    want = u8.permute(2, 0, 1).float().div(255)
    assert torch.equal(C.to_tensor64(u8).float(), want)
    assert float((C.to_tensor64(u8) - want.double()).abs().max()) <= 2.0 ** -25  # half an ulp below 1


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_every_case_keeps_the_relu_margin(case):
    """No case and no row is excused for a ReLU flip: every hidden pre-activation of the float64 model is RELU_MARGIN from 0."""
    w, b, *_ = C.params64(C.reference_mlp(case))
    x = C.inputs(case)
    assert x.dtype == torch.float32 and torch.equal((x * 255).round() / 255, x)  # u8 / 255 values
    assert C.min_hidden_margin(x, w, b) >= C.RELU_MARGIN
    assert C.max_layer_norm_gain(x, w, b) <= C.LN_GAIN_MAX  # two logits that nearly tie would turn 1e-7 into 1e-5 behind the norm


# ---------------------------------------------------------------- the golden against the formulas
def _golden_model_and_batches():
    from graphnet_classifier_amd.MLP import MLP
    g = load_golden("g12_image_mlp.npz")
    side = int(g["side"])
    torch.manual_seed(int(g["model_seed"]))
    model = MLP(3 * side * side, 2).cpu().double()
    x = torch.stack([C.to_tensor64(torch.from_numpy(r)).float() for r in g["resized"]])  # float32, as ToTensor stores it
    return g, model, x, torch.from_numpy(g["labels"])


def _cross_entropy64(logits, labels):
    """mean over the batch of -log softmax(logits)[label], and its gradient (softmax - onehot) / B"""
    z = logits.double()
    lse = torch.logsumexp(z, dim=1)
    loss = (lse - z[torch.arange(len(labels)), labels]).mean()
    grad = torch.softmax(z, dim=1)
    grad[torch.arange(len(labels)), labels] -= 1.0
    return loss, grad / len(labels)


def test_golden_fixture_is_consistent():
    from PIL import Image
    g = load_golden("g12_image_mlp.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g12_image_mlp.npz")) < 1 << 20
    assert not any("weight" in k and "grad/" not in k for k in g)  # seeds, not weight matrices
    photos = [g[f"photo_{i:02d}"] for i in range(len(g["labels"]))]
    side = int(g["side"])
    for p, r in zip(photos, g["resized"]):
        assert np.array_equal(np.array(Image.fromarray(p).resize((side, side), Image.Resampling.BILINEAR)), r)
    n, b = len(photos), int(g["batch_size"])
    assert len(g["step_losses"]) == int(g["epochs"]) * -(-n // b) and n % b != 0  # a short last batch in every epoch
    torch.manual_seed(int(g["loader_seed"]))
    first = next(iter(torch.utils.data.DataLoader(list(range(n)), batch_size=b, shuffle=True)))
    assert np.array_equal(first.numpy(), g["first_batch_indices"])
    assert np.array_equal(g["labels"][g["first_batch_indices"]], g["first_batch_labels"])


def test_golden_first_step_equals_formulas():
    g, model, x, labels = _golden_model_and_batches()
    idx = torch.from_numpy(g["first_batch_indices"])
    w, b, gamma, beta, eps = C.params64(model)
    xb = x[idx].reshape(len(idx), -1)
    logits, *_ = C.forward64(xb, w, b, gamma, beta, eps)
    assert float((logits - torch.from_numpy(g["first_batch_logits"]).double()).abs().max()) < 1e-5
    loss, dlogits = _cross_entropy64(logits, labels[idx])
    assert abs(float(loss) - float(g["step_losses"][0])) < 1e-5
    grads = C.backward64(xb, w, b, gamma, beta, eps, dlogits)
    named = {"model.0.bias": grads["b"][0], "model.2.weight": grads["w"][1], "model.2.bias": grads["b"][1],
             "model.4.weight": grads["w"][2], "model.4.bias": grads["b"][2], "model.5.weight": grads["gamma"], "model.5.bias": grads["beta"]}
    assert sorted("grad/" + k for k in named) == sorted(k for k in g if k.startswith("grad/"))
    for k, v in named.items():
        ref = torch.from_numpy(g["grad/" + k]).double()
        assert float((v - ref).abs().max()) <= 2e-5 + 1e-4 * float(ref.abs().max()), k


def test_golden_float64_run_repeats():
    """The 3 epochs again in float64 (torch.nn modules, Adam, the DataLoader's batches) equal the float64 losses the fixture stores
    next to the reference's float32 ones, and the reference's float32 run is within 1e-6 of them (4e-7 when captured): fp32
    rounding does not decide this run, so the 1e-5 that train() is held to on the GPU is a bound on the code, not on luck."""
    g, model, x, labels = _golden_model_and_batches()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    torch.manual_seed(int(g["loader_seed"]))
    loader = torch.utils.data.DataLoader(list(range(len(labels))), batch_size=int(g["batch_size"]), shuffle=True)
    got = []
    for _ in range(int(g["epochs"])):
        total, steps = 0.0, 0
        for idx in loader:
            loss = torch.nn.functional.cross_entropy(model.model(x[idx].reshape(len(idx), -1).double()), labels[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
            total, steps = total + float(loss.detach()), steps + 1
        got.append(total / steps)
    assert np.abs(np.array(got) - g["epoch_losses_float64"]).max() < 1e-9
    assert np.abs(g["epoch_losses"] - g["epoch_losses_float64"]).max() < 1e-6
    per = len(g["step_losses"]) // int(g["epochs"])
    assert np.abs(g["step_losses"].reshape(-1, per).mean(axis=1) - g["epoch_losses"]).max() < 1e-12


# ---------------------------------------------------------------- loader order
def test_tensor_loader_index_batches_follow_dataloader(tmp_path):
    for k in range(19):
        p = tmp_path / f"c{k % 2}" / f"img{k:02d}.png"
        p.parent.mkdir(exist_ok=True)
        p.write_bytes(b"")
    ds = D.ImageTensorFolder(str(tmp_path), resize_value=20)
    assert len(ds) == 19 and ds.classes == ["c0", "c1"] and ds.targets == [0] * 10 + [1] * 9
    for shuffle, drop_last in [(True, False), (True, True), (False, False)]:
        torch.manual_seed(123)
        want = [b.tolist() for b in torch.utils.data.DataLoader(list(range(19)), batch_size=8, shuffle=shuffle, drop_last=drop_last)]
        after_want = torch.rand(1)
        torch.manual_seed(123)
        loader = ds.loader(batch_size=8, shuffle=shuffle, drop_last=drop_last)
        got = loader.index_batches()
        assert got == want and len(loader) == len(want)
        assert torch.equal(torch.rand(1), after_want)  # the same draws from the global RNG
    assert ds.loader().batch_size == 8 and ds.loader().shuffle is True  # main.py:17


# ---------------------------------------------------------------- C ABI
def test_new_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    lib = native.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in native._SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gnc_abi_version() == 20 and "#define GNC_ABI_VERSION 20" in header


def _desc(rows, K, H, layers, segments=None, residual=False, activation="ReLU"):
    x = torch.empty(rows, K)
    weights = [torch.empty(H, K)] + [torch.empty(H, H) for _ in range(layers - 1)] + [torch.empty(2, H)]
    biases = [torch.empty(w.size(0)) for w in weights]
    segs = segments(x) if segments else [(x, None, K, native.SEG_MATMUL, 0)]
    out = torch.empty(rows, 2)
    keep = (x, weights, biases, segs, out)
    return native.make_mlp_desc(segs, weights, biases, None, activation, 0.0, out if residual else None, out, rows), keep


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_wide_linear_supported_takes_every_case(case):
    rows, K, H, layers = case
    desc, keep = _desc(rows, K, H, layers)
    plan = native.wide_linear_plan_of(desc)
    assert plan is not None
    s, n = plan["k_slices"], plan["k_slice_len"]
    assert n % 32 == 0 and s >= 1 and (s - 1) * n < K <= s * n  # the slices [i n, min((i + 1) n, K)) cover K exactly once
    r, p = plan["dw_row_range"], plan["dw_parts"]
    assert r % 16 == 0 and (p - 1) * r < rows <= p * r
    lib = native.load_library()
    assert plan["forward_workspace_floats"] == lib.gnc_wide_linear_workspace_floats(rows, K, H, 0) == s * rows * ((H + 15) // 16 * 16)
    assert plan["backward_workspace_floats"] == lib.gnc_wide_linear_workspace_floats(rows, K, H, 1)
    assert (plan["backward_workspace_floats"] == 0) == (p == 1)


def test_wide_linear_supported_refusals():
    lib = native.load_library()
    refused = lambda d: native.wide_linear_plan_of(d[0]) is None  # noqa: E731
    assert not refused(_desc(8, 1024, 128, 2)) and not refused(_desc(8, 1024, 256, 2)) and not refused(_desc(8, 1024, 1, 2))
    assert refused(_desc(8, 1023, 128, 2))   # K < 1024: the row-tiled kernels keep it
    assert refused(_desc(8, 768, 128, 2))    # (the graph model's widest first Linear)
    assert refused(_desc(8, 2048, 257, 2))   # wider than 256
    assert refused(_desc(8, 2048, 128, 2, residual=True))
    two = lambda x: [(x[:, :1024], None, 1024, native.SEG_MATMUL, 0), (x[:, 1024:], None, 1024, native.SEG_MATMUL, 1024)]  # noqa: E731
    assert refused(_desc(8, 2048, 128, 2, segments=two))
    index = torch.zeros(8, dtype=torch.int32)
    assert refused(_desc(8, 2048, 128, 2, segments=lambda x: [(x, index, 2048, native.SEG_MATMUL, 0)]))
    assert refused(_desc(8, 2048, 128, 2, segments=lambda x: [(x, None, 2048, native.SEG_ADD, 0)]))
    one_linear, keep = _desc(8, 2048, 128, 2)
    one_linear.num_linear = 1
    assert native.wide_linear_plan_of(one_linear) is None
    assert lib.gnc_wide_linear_supported(None, None) == 0
    assert lib.gnc_wide_linear_workspace_floats(0, 2048, 128, 0) == -1 and lib.gnc_wide_linear_workspace_floats(8, 1023, 128, 1) == -1
