"""GPU: the image-MLP baseline end to end - MLP(...) through the K16 route against the float64 formulas, the route's launches and
its A/B switch, ToTensor and the tensor loader against Pillow, train() on tensor batches against the golden captured from the
reference (tests/golden/g12_image_mlp.npz), the captured tensor step against the eager one, and mlp_inference."""
import ast
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from graphnet_classifier_amd import baseline, native
from graphnet_classifier_amd import dataset as D
from graphnet_classifier_amd import functional as Fn
from graphnet_classifier_amd.MLP import MLP
from graphnet_classifier_amd.train import CapturedTensorStep, FlatParameters, FusedAdam, train
from tests import image_mlp_cases as C
from tests._util import load_golden, sub_state_dict, t

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _launch_names(fn):
    names = []
    native.set_kernel_timers(type("T", (), {"launch": lambda self, name, t, f, work=0.0: (names.append(name), f())[1]})())
    try:
        out = fn()
    finally:
        native.set_kernel_timers(None)
    return out, names


@functools.lru_cache(maxsize=None)
def _reference(case, norm_type):
    model = C.reference_mlp(case, "ReLU", norm_type)
    p = C.params64(model)
    x, g = C.inputs(case), C.cotangent(case)
    out, *_ = C.forward64(x, *p)
    return model.state_dict(), x, g, out, C.backward64(x, *p, g)


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max())


@pytest.mark.parametrize("norm_type", ["LayerNorm", None])
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_mlp_through_the_route_equals_formulas(case, norm_type, monkeypatch):
    monkeypatch.delenv("GNC_NO_WIDE_LINEAR", raising=False)
    sd, x, g, out_ref, grads = _reference(case, norm_type)
    rows, K, H, layers = case
    model = MLP(K, 2, hidden_dim=H, hidden_layers=layers, norm_type=norm_type)
    model.load_state_dict(sd)
    xd = x.to(DEV)
    out, names = _launch_names(lambda: model(xd))
    assert names[0] == f"wide_linear_forward_in{K}_h{H}" and len(names) == 2 and names[1].startswith(f"mlp_fused_in{H}_")
    e_out = _err(out, out_ref)
    _, names = _launch_names(lambda: out.backward(g.to(DEV)))
    assert f"wide_linear_backward_in{K}_h{H}" in names
    lin = [m for m in model.model if isinstance(m, torch.nn.Linear)]
    worst = {}
    for k, m in enumerate(lin):
        for got, ref, tag in ((m.weight.grad, grads["w"][k], f"dW{k}"), (m.bias.grad, grads["b"][k], f"db{k}")):
            e, bound = _err(got, ref), 2e-5 + 1e-4 * float(ref.abs().max())
            worst[tag] = (e, bound)
    if norm_type is not None:
        for got, ref, tag in ((model.model[-1].weight.grad, grads["gamma"], "dgamma"), (model.model[-1].bias.grad, grads["beta"], "dbeta")):
            worst[tag] = (_err(got, ref), 2e-5 + 1e-4 * float(ref.abs().max()))
    print(f"\nroute {C.case_id(case)} {norm_type}: out {e_out:.2e} (bound {1e-5 * max(1.0, float(out_ref.abs().max())):.2e}) "
          + " ".join(f"{k} {e:.1e}/{b:.1e}" for k, (e, b) in worst.items()))
    assert e_out <= 1e-5 * max(1.0, float(out_ref.abs().max()))
    for tag, (e, bound) in worst.items():
        assert e <= bound, (tag, e, bound)
    # route off: the row-tiled kernels, another launch name, the same values within the forward bound
    monkeypatch.setenv("GNC_NO_WIDE_LINEAR", "1")
    with torch.no_grad():
        off, names_off = _launch_names(lambda: model(xd))
    assert names_off == [f"mlp_fused_in{K}_h{H}_out2_L{layers + 1}"]
    assert _err(off, out.detach().double().cpu()) <= 1e-5 * max(1.0, float(out_ref.abs().max()))
    assert _err(off, out_ref) <= 1e-5 * max(1.0, float(out_ref.abs().max()))


def test_route_conditions(monkeypatch):
    monkeypatch.delenv("GNC_NO_WIDE_LINEAR", raising=False)
    x = torch.rand(8, 2048, device=DEV)
    w = [torch.randn(128, 2048, device=DEV) * 0.02, torch.randn(2, 128, device=DEV)]
    b = [torch.zeros(128, device=DEV), torch.zeros(2, device=DEV)]
    assert Fn.wide_linear_route([(x, None)], w, b, None, "ReLU", None, None)
    assert not Fn.wide_linear_route([(x[:, :1000], None)], [w[0][:, :1000], w[1]], b, None, "ReLU", None, None)  # K < 1024
    assert not Fn.wide_linear_route([(x, None)], w, b, None, "ReLU", torch.zeros(8, 2, device=DEV), None)      # residual
    assert not Fn.wide_linear_route([(x, torch.arange(8, dtype=torch.int32, device=DEV))], w, b, None, "ReLU", None, None)  # gathered
    assert not Fn.wide_linear_route([(x[:, :1024], None), (x[:, 1024:], None)], w, b, None, "ReLU", None, None)
    assert not Fn.wide_linear_route([(x.clone().requires_grad_(True), None)], w, b, None, "ReLU", None, None)   # dx is not formed
    assert not Fn.wide_linear_route([(x, None)], w[:1], b[:1], None, "ReLU", None, None)                          # a single Linear
    monkeypatch.setenv("GNC_NO_WIDE_LINEAR", "1")
    assert not Fn.wide_linear_route([(x, None)], w, b, None, "ReLU", None, None)


@pytest.mark.parametrize("activation,norm_type", [("GELU", "LayerNorm"), ("Identity", None), ("ReLU", "BatchNorm1d")])
def test_other_activations_and_batchnorm_through_the_route(activation, norm_type, monkeypatch):
    """The z0 the tail stores feeds the layer-by-layer backward of a non-ReLU chain; BatchNorm1d takes the route for its Linear
    chain.  Reference: the same modules in float64 on the host."""
    monkeypatch.delenv("GNC_NO_WIDE_LINEAR", raising=False)
    case = (17, 3072, 128, 2)
    model = C.reference_mlp(case, activation, norm_type)
    ref = torch.nn.Sequential(*[type(m)(m.in_features, m.out_features) if isinstance(m, torch.nn.Linear) else
                                (type(m)(2) if isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm1d)) else type(m)())
                                for m in model.model]).double()
    ref.load_state_dict({k[len("model."):]: v.detach().cpu().double() if v.is_floating_point() else v.cpu()
                         for k, v in model.state_dict().items()})
    x, g = C.inputs(case), C.cotangent(case)
    want = ref(x.double())
    want.backward(g.double())
    out, names = _launch_names(lambda: model(x.to(DEV)))
    assert names[0] == "wide_linear_forward_in3072_h128"
    out.backward(g.to(DEV))
    assert _err(out, want.detach()) <= 1e-5 * max(1.0, float(want.abs().max()))
    for (n, p), q in zip(model.model.named_parameters(), ref.parameters()):
        assert _err(p.grad, q.grad) <= 2e-5 + 1e-4 * float(q.grad.abs().max()), n


def test_graphnet_forward_does_not_see_the_route(monkeypatch):
    from graphnet_classifier_amd import GNN as G
    g = load_golden("g4_graphnet_tiny.npz")
    m = G.GraphNet(**ast.literal_eval(bytes(g["kwargs_json"]).decode()))
    m.load_state_dict(sub_state_dict(g, "sd/"), strict=True)
    outs, launches = [], []
    for off in (False, True):
        monkeypatch.setenv("GNC_NO_WIDE_LINEAR", "1") if off else monkeypatch.delenv("GNC_NO_WIDE_LINEAR", raising=False)
        with torch.no_grad():
            y, names = _launch_names(lambda: m(t(g["x"], DEV), t(g["pos"], DEV), t(g["edge_index"], DEV)))
        outs.append(y)
        launches.append(names)
    assert torch.equal(outs[0], outs[1]) and launches[0] == launches[1]
    assert not any(n.startswith("wide_linear") for n in launches[0])


# ---------------------------------------------------------------- ToTensor and the loader
@pytest.mark.parametrize("shape", [(3, 20, 20, 3), (64, 128, 128, 3), (2, 5, 7, 1)])
def test_u8_hwc_to_f32_chw_is_permute_float_div(shape):
    gen = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    n = min(256, img.numel())
    img.view(-1)[:n] = torch.arange(n, dtype=torch.uint8)  # every byte value where the batch has room
    got = native.u8_hwc_to_f32_chw(img.to(DEV))
    want = torch.stack([im.permute(2, 0, 1).float().div(255) for im in img])
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got.cpu(), want)


@pytest.fixture(scope="module")
def golden_folder(tmp_path_factory):
    g = load_golden("g12_image_mlp.npz")
    root = tmp_path_factory.mktemp("image_mlp")
    for i, label in enumerate(g["labels"]):
        d = root / ("chihuahua" if label == 0 else "muffin")
        d.mkdir(exist_ok=True)
        Image.fromarray(g[f"photo_{i:02d}"]).save(d / f"img{i:02d}.png")
    return str(root), g


def test_loader_first_batch_equals_pillow_bilinear(golden_folder):
    root, g = golden_folder
    ds = D.ImageTensorFolder(root, resize_value=int(g["side"]))
    assert ds.classes == ["chihuahua", "muffin"] and ds.targets == g["labels"].tolist()
    torch.manual_seed(int(g["loader_seed"]))
    batches = list(ds.loader(batch_size=8))
    assert [len(y) for _, y in batches] == [8, 8, 3]
    x, y = batches[0]
    idx = g["first_batch_indices"]
    want = torch.stack([torch.from_numpy(np.array(Image.open(ds.samples[i][0]).convert("RGB").resize((20, 20), Image.Resampling.BILINEAR)))
                        .permute(2, 0, 1).float().div(255) for i in idx])
    assert x.is_cuda and x.dtype == torch.float32 and torch.equal(x.cpu(), want)
    assert torch.equal(want, torch.stack([C.to_tensor64(torch.from_numpy(g["resized"][i])).float() for i in idx]))
    assert y.dtype == torch.long and y.tolist() == g["first_batch_labels"].tolist()
    item, label = ds[int(idx[0])]
    assert torch.equal(item, x[0]) and label == int(y[0])
    loader = baseline.load_data(root, 20, 8)
    assert loader.batch_size == 8 and loader.shuffle and loader.dataset.classes == ds.classes


# ---------------------------------------------------------------- training
def _golden_run(root, g, capture, tmp):
    torch.manual_seed(int(g["model_seed"]))
    model = MLP(3 * int(g["side"]) ** 2, 2)
    torch.manual_seed(int(g["loader_seed"]))
    loader = D.ImageTensorFolder(root, resize_value=int(g["side"])).loader(batch_size=int(g["batch_size"]))
    history = train(model, loader, int(g["epochs"]), output_path=str(tmp), capture=capture)
    return model, history


def test_train_reproduces_the_reference_epoch_losses(golden_folder, tmp_path):
    """train(MLP(1200, 2), ImageTensorFolder(...).loader(batch_size=8), 3) against the reference's own run, within the 1e-5 the G8
    training-run golden is held to.  The first batch's logits (before any update) are compared as well."""
    root, g = golden_folder
    torch.manual_seed(int(g["model_seed"]))
    model = MLP(1200, 2)
    ds = D.ImageTensorFolder(root, resize_value=20)
    torch.manual_seed(int(g["loader_seed"]))
    x, y = next(iter(ds.loader(batch_size=8)))
    with torch.no_grad():
        logits = model(x)
    e0 = float((logits.cpu() - torch.from_numpy(g["first_batch_logits"])).abs().max())
    model, history = _golden_run(root, g, True, tmp_path)
    gaps = np.abs(np.array(history["avg_loss"]) - g["epoch_losses"])
    print(f"\nfirst-batch logits {e0:.2e}; epoch losses {history['avg_loss']} vs reference {g['epoch_losses'].tolist()} "
          f"(float64 run {g['epoch_losses_float64'].tolist()}): gaps {gaps.tolist()}")
    assert e0 < 1e-5
    assert history["captured_tensor"] is True
    assert gaps.max() < 1e-5


def test_captured_and_eager_runs_are_bitwise_equal(golden_folder, tmp_path):
    root, g = golden_folder
    out = {}
    for capture in (True, False):
        model, history = _golden_run(root, g, capture, tmp_path / str(capture))
        assert history["captured_tensor"] is capture and history["captured"] is False and history["batched"] is False
        assert len(history["avg_loss"]) == 3  # 8 + 8 + 3 images per epoch: the short last batch ran (eagerly) in both
        out[capture] = ({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, history["avg_loss"])
    assert out[True][1] == out[False][1]
    for k, v in out[True][0].items():
        assert torch.equal(v, out[False][0][k]), k


def test_constructing_the_capture_does_not_train(golden_folder):
    root, g = golden_folder
    torch.manual_seed(1)
    model = MLP(1200, 2, norm_type="BatchNorm1d")
    opt = FusedAdam(FlatParameters(model), lr=1e-3)
    loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
    x, y = next(iter(D.ImageTensorFolder(root, resize_value=20).loader(batch_size=8, shuffle=False)))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    adam = [s.clone() for s in opt.state_snapshot()]
    step = CapturedTensorStep(model, opt, torch.nn.CrossEntropyLoss(), x, y, loss_sum)
    assert float(loss_sum.item()) == 0.0
    for k, v in model.state_dict().items():  # parameters and the BatchNorm buffers
        assert torch.equal(before[k], v), k
    for a, b in zip(adam, opt.state_snapshot()):
        assert torch.equal(a, b)
    assert step.matches(x, y) and not step.matches(x[:3], y[:3]) and not step.matches(x.double(), y)
    step(x, y)
    assert float(loss_sum.item()) > 0 and int(opt.step_count.item()) == 1
    assert any(not torch.equal(before[k], v) for k, v in model.state_dict().items())


def test_other_modules_on_tensor_samples_keep_the_eager_step(tmp_path):
    """Only this package's MLP is captured: another module may read host state in its forward, which a replay would not repeat."""
    torch.manual_seed(0)
    module = torch.nn.Linear(12, 2).to(DEV)
    dataset = [(torch.rand(4, 12), torch.randint(0, 2, (4,))) for _ in range(3)]
    history = train(module, dataset, 1, output_path=str(tmp_path))
    assert history["captured_tensor"] is False and len(history["avg_loss"]) == 1


# ---------------------------------------------------------------- inference
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_mlp_inference_equals_formula_on_pillow_pixels(tmp_path, mode):
    g = load_golden("g12_image_mlp.npz")
    path = str(tmp_path / "photo.jpg")
    Image.fromarray(g["photo_03"]).convert(mode).save(path, quality=90)
    side = 24
    torch.manual_seed(4)
    model = MLP(side * side * 3, 2)
    weights = str(tmp_path / "final_model.pth")
    torch.save({k: v.cpu() for k, v in model.state_dict().items()}, weights)
    pixels = np.array(Image.open(path).resize((side, side)).convert("RGB"))  # Pillow's own, in the reference's order
    assert torch.equal(baseline.inference_pixels(path, side).cpu(), torch.from_numpy(pixels))
    x = torch.from_numpy(pixels.flatten()).float().unsqueeze(0)  # raw 0 ... 255 values, H W C order
    want, *_ = C.forward64(x, *C.params64(model))
    logits, prob = baseline.mlp_inference(path, weights, side)
    assert logits.shape == (1, 2) and _err(logits, want) <= 1e-5 * max(1.0, float(want.abs().max()))
    assert _err(prob, torch.softmax(want, dim=1)) <= 1e-5
