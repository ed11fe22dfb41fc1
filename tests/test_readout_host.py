"""Host side of the single-graph read-out tests (no GPU): the float64 formulas of tests/readout_cases.py against
torch.nn.Linear + autograd, the ReLU-kink condition of every case with none left out, the plain fp32 CPU evaluation within the
bars the GPU test holds the kernels to, and the exported symbols."""
import itertools
import os
import re

import pytest
import torch

from graphnet_classifier_amd import native
from tests import readout_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gnc_readout_forward_f32", "gnc_readout_backward_f32", "gnc_adam_step_f32")
BIAS_COMBOS = list(itertools.product((True, False), repeat=3))


def _torch_nn(c):
    """(logits, h1, h2, gradients in the order of R.GRADS) from float64 torch.nn.Linear modules and autograd."""
    y = c["y"].clone().requires_grad_(True)
    fcs = []
    for k in (1, 2, 3):
        w, b = c[f"w{k}"], c[f"b{k}"]
        fc = torch.nn.Linear(w.size(1), w.size(0), bias=b is not None, dtype=torch.float64)
        with torch.no_grad():
            fc.weight.copy_(w)
            if b is not None:
                fc.bias.copy_(b)
        fcs.append(fc)
    h1 = torch.relu(fcs[0](y))
    h2 = torch.relu(fcs[1](h1))
    logits = fcs[2](h2)
    logits.backward(c["g"])
    grads = [y.grad] + [t for fc in fcs for t in (fc.weight.grad, fc.bias.grad if fc.bias is not None else None)]
    return logits.detach(), h1.detach(), h2.detach(), grads


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.case_id)
def test_formulas_equal_torch_nn_float64(shape):
    c = R.build(shape)
    out = R.evaluate(c)
    logits, h1, h2, grads = _torch_nn(c)
    for name, want in zip(R.OUTPUTS + R.GRADS, [logits, h1, h2] + grads):
        assert out[name].shape == want.shape and out[name].dtype == torch.float64, name
        assert _rel(out[name], want) <= 1e-12, name


@pytest.mark.parametrize("keep", BIAS_COMBOS, ids=lambda k: "b" + "".join(str(int(v)) for v in k))
def test_formulas_without_biases_equal_torch_nn_float64(keep):
    c = R.without_biases(R.build(R.BIAS_SHAPE), keep)
    out = R.evaluate(c)
    logits, h1, h2, grads = _torch_nn(c)
    for name, want in zip(R.OUTPUTS + R.GRADS, [logits, h1, h2] + grads):
        if want is not None:  # the gradient of an absent bias: the kernel still writes dz, the formulas return it
            assert _rel(out[name], want) <= 1e-12, name


def test_inputs_are_fp32_representable_and_follow_the_recipe():
    for shape in R.SHAPES:
        c = R.build(shape)
        F, H1, H2, C = shape
        assert [tuple(c[k].shape) for k in R.INPUTS] == [(F,), (H1, F), (H1,), (H2, H1), (H2,), (C, H2), (C,), (C,)]
        for k, v in c.items():
            assert v.dtype == torch.float64 and torch.equal(v.float().double(), v), k
    c = R.build((4096, 128, 32, 2))
    assert abs(float(c["w1"].std()) * 4096 ** 0.5 - 1.0) < 0.02 and abs(float(c["y"].std()) - 1.0) < 0.05
    assert abs(float(c["b1"].std()) - 0.1) < 0.03


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.case_id)
def test_every_case_keeps_its_distance_from_the_relu_kink(shape):
    """No case and no unit is excused: min|z| >= KINK rms(z) for both pre-activations, and the fp32 evaluation draws the same
    masks, so every gradient element is compared."""
    r = R.reference_of(shape)
    for z in ("z1", "z2"):
        assert R.kink_ratio(r["ref"][z]) >= R.KINK, z
        assert float((r["fp32"][z].double() - r["ref"][z]).abs().max()) < 0.01 * R.KINK * float(r["ref"][z].pow(2).mean().sqrt())
    for h in ("h1", "h2"):
        assert torch.equal(r["fp32"][h] > 0, r["ref"][h] > 0), h
    assert set(R.SEEDS) == set(R.SHAPES) and len(R.SHAPES) == 9


def _within(r):
    for name in R.OUTPUTS + R.GRADS:
        ref, bar = r["ref"][name], r["bar"][name]
        assert bar >= R.BAR_FACTOR * R.ULP * float(ref.abs().max()) and bar >= R.BAR_FACTOR * r["err"][name], name
        assert bar <= 1e-4 * float(ref.abs().max()) or float(ref.abs().max()) == 0.0, name  # a bar, not an excuse
        assert R.max_err(r["fp32"][name], ref) <= bar, name


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.case_id)
def test_fp32_cpu_evaluation_meets_the_bars(shape):
    _within(R.reference_of(shape))


def test_fp32_cpu_evaluation_meets_the_bars_without_biases_and_on_the_relu_edges():
    for keep in BIAS_COMBOS:
        _within(R.reference_of(R.BIAS_SHAPE, keep))
    c = R.relu_edge_case()
    r = R.reference(c)
    _within(r)
    units = list(R.EDGE_UNITS)
    assert torch.equal(r["ref"]["z1"][units], torch.tensor(list(R.EDGE_UNITS.values()), dtype=torch.float64))
    assert float(r["ref"]["h1"][units].abs().max()) == 0.0 and float(r["ref"]["db1"][units].abs().max()) == 0.0
    assert float(r["ref"]["dW1"][units].abs().max()) == 0.0


@pytest.mark.parametrize("shape", R.OVER_LIMIT + ((257, 65, 33, 5), (1024, 257, 1024, 63)), ids=R.case_id)
def test_any_order_bound_holds_for_fp32_on_the_cpu_in_several_orders(shape):
    """The bar of the over-limit widths' torch path: torch's fp32 GEMV, the same sums taken backwards and a plain sequential
    loop all stay inside it, and it stays a statement about fp32 (below 1e-4 of the largest logit)."""
    c = R.over_limit_case(shape) if shape in R.OVER_LIMIT else R.build(shape)
    ref, bound = R.evaluate(c)["logits"], R.any_order_logits_bound(c)
    assert bound.shape == ref.shape and float(bound.max()) <= 1e-4 * float(ref.abs().max()) and float(bound.min()) > 0
    flipped = {k: (v.flip(-1) if k.startswith("w") else v) for k, v in c.items()}
    flipped["y"] = c["y"].flip(0)
    f = {k: v.float() for k, v in flipped.items()}
    h1 = torch.relu(f["w1"] @ f["y"] + f["b1"]).flip(0)
    h2 = torch.relu(f["w2"] @ h1 + f["b2"]).flip(0)
    backwards = f["w3"] @ h2 + f["b3"]
    a = {k: v.float() for k, v in c.items()}
    seq = lambda w, h, b: torch.stack([torch.cumsum(w[r] * h, 0)[-1] for r in range(w.size(0))]) + b  # noqa: E731
    sequential = seq(a["w3"], torch.relu(seq(a["w2"], torch.relu(seq(a["w1"], a["y"], a["b1"])), a["b2"])), a["b3"])
    for got in (R.evaluate(c, torch.float32)["logits"], backwards, sequential):
        assert bool(((got.double() - ref).abs() <= bound).all())


def test_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    lib = native.load_library()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in native._SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gnc_abi_version() == native.ABI_VERSION
    assert (native.READOUT_MAX_HIDDEN, native.READOUT_MAX_CLASSES) == (1024, 64)
