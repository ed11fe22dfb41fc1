"""The three row-wise kernels of csrc/elementwise.hip, each directly against float64 (inputs, definitions and bars:
tests/elementwise_cases.py): gnc_activation_f32 and gnc_activation_backward_f32 for every activation but ReLU on one input
table that covers the cancellation range near 0 and the overflow range of expf, at widths 1 .. 256, with operands that are
column slices of wider tensors (ld > width) and with more elements than the capped grid has threads;
gnc_layer_norm_backward_f32 at widths below, at and above one wave per row, with more rows than the grid has waves, with
ld > width on all four tensors, on rows around 1e3 and on constant rows.

ELU: with ``p * (expf(x) - 1.f)`` (the form before this file existed) the relative figure of the forward was 1.0 on an
MI355X and 1.1 in fp32 on the CPU (-1e-8 came out as 0); with ``p * expm1f(x)`` it is 5.6e-8 on an MI355X, 6.0e-8 on the CPU.
Worst figures on an MI355X over all six activations: 1.1e-7 of max(1, |x|) and 1.9e-7 of |ref| (SiLU), as on the CPU."""
import pytest
import torch

from tests import elementwise_cases as E

DEV = "cuda:0"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from graphnet_classifier_amd import native as n
    n.load_library()
    return n


def _cu() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _wide(t: torch.Tensor):
    """``t`` on the device as columns [4, 4 + width) of a tensor 8 columns wider, whose other columns hold 7.0."""
    wide = torch.full((t.size(0), t.size(1) + 8), 7.0, dtype=torch.float32, device=DEV)
    wide[:, 4:4 + t.size(1)] = t.to(DEV)
    return wide, wide[:, 4:4 + t.size(1)]


def _untouched(wide: torch.Tensor, width: int) -> bool:
    return bool((wide[:, :4] == 7.0).all() and (wide[:, 4 + width:] == 7.0).all())


def _table(width: int, reps: int = 1):
    x = E.table().repeat(reps).reshape(-1, width)
    return x, E.grad_table(x.numel()).reshape(-1, width)


def _check(name, what, got, ref, x, scale=None):
    e = E.errors(got.cpu(), ref, x, scale)
    print(f"{name} {what} [{x.size(0)} x {x.size(1)}]: abs {e['abs']:.2e} of max(1, |x|) (bar {E.ABS_BAR:.0e}), "
          f"rel on |x| <= {E.REL_RANGE:.0e} {e['rel']:.2e} (bar {E.REL_BAR:.0e})")
    assert e["finite"], (name, what)
    assert e["abs"] <= E.ABS_BAR, (name, what)
    assert e["rel"] <= E.REL_BAR, (name, what)


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("width", E.WIDTHS)
@pytest.mark.parametrize("name,param", E.ACTS)
def test_activation_and_derivative_against_float64(native, name, param, width):
    x, da = _table(width)
    ref_a, ref_d = E.reference(x, name, param)
    xd, dad = x.to(DEV), da.to(DEV)
    a = native.activation(xd, name, param)
    dz = native.activation_backward(xd, dad, name, param)
    _check(name, "forward", a, ref_a, x)
    _check(name, "backward", dz, ref_d * da.double(), x, scale=da)
    # the same through column slices of wider tensors: input, gradient and output
    (_, xs), (_, das) = _wide(x), _wide(da)
    (wa, oa), (wd, od) = _wide(torch.zeros_like(x)), _wide(torch.zeros_like(x))
    assert native.activation(xs, name, param, out=oa) is oa and native.activation_backward(xs, das, name, param, out=od) is od
    assert torch.equal(oa, a) and torch.equal(od, dz)
    assert _untouched(wa, width) and _untouched(wd, width)


@pytest.mark.parametrize("name,param", E.ACTS)
def test_activation_with_more_elements_than_the_grid_has_threads(native, name, param):
    """grid_for caps the grid at 16 blocks of 256 threads per CU: the table repeated until it is longer than that."""
    reps = (16 * 256 * _cu()) // E.TABLE_LEN + 2
    x, da = _table(256, reps)
    assert x.numel() > 16 * 256 * _cu()
    ref_a, ref_d = E.reference(x, name, param)
    xd, dad = x.to(DEV), da.to(DEV)
    a, dz = native.activation(xd, name, param), native.activation_backward(xd, dad, name, param)
    _check(name, "forward", a, ref_a, x)
    _check(name, "backward", dz, ref_d * da.double(), x, scale=da)
    assert torch.equal(native.activation(xd, name, param), a) and torch.equal(native.activation_backward(xd, dad, name, param), dz)


@pytest.mark.parametrize("name,param", E.ACTS)
def test_nan_stays_nan(native, name, param):
    """A NaN input gives NaN, and so does its derivative; LeakyReLU's derivative is one of two constants and takes the slope,
    as PyTorch's does."""
    x = torch.tensor([[float("nan"), 1.0, float("nan"), -1.0, 0.0]])
    a = native.activation(x.to(DEV), name, param).cpu()
    assert torch.equal(torch.isnan(a), torch.isnan(x))
    dz = native.activation_backward(x.to(DEV), torch.ones_like(x).to(DEV), name, param).cpu()
    if name == "LeakyReLU":
        assert torch.equal(dz, torch.tensor([[param, 1.0, param, param, param]]))
    else:
        assert torch.equal(torch.isnan(dz), torch.isnan(x))


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_rows(key: str) -> int:
    return {"one": 1, "few": 37, "waves": 64 * _cu() + 37}[key]  # waves: more rows than 16 blocks x 4 waves per CU


def _ln_case(native, rows, width, kind):
    y, gamma, g = E.ln_inputs(rows, width, kind)
    ref_dy, ref_yh = E.ln_reference(y, gamma, g)
    bar_dy, bar_yh = E.ln_bars(kind, ref_yh)
    yd, gd, gm = y.to(DEV), g.to(DEV), gamma.to(DEV)
    dy, yh = native.layer_norm_backward(yd, gm, gd, E.LN_EPS)
    e_dy, e_yh = float((dy.double().cpu() - ref_dy).abs().max()), float((yh.double().cpu() - ref_yh).abs().max())
    print(f"layer_norm_backward {kind} [{rows} x {width}]: dy {e_dy:.2e} (bar {bar_dy:.1e}), y_hat {e_yh:.2e} (bar {bar_yh:.1e})")
    assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(yh).all())
    assert e_dy < bar_dy and e_yh < bar_yh
    dy2, yh2 = native.layer_norm_backward(yd, gm, gd, E.LN_EPS)
    assert torch.equal(dy2, dy) and torch.equal(yh2, yh)
    # ld > width on y, grad_out, dy and y_hat
    (_, ys), (_, gs) = _wide(y), _wide(g)
    (w1, o1), (w2, o2) = _wide(torch.zeros_like(y)), _wide(torch.zeros_like(y))
    native.layer_norm_backward(ys, gm, gs, E.LN_EPS, out=(o1, o2))
    assert torch.equal(o1, dy) and torch.equal(o2, yh)
    assert _untouched(w1, width) and _untouched(w2, width)


@pytest.mark.parametrize("key", ["one", "few", "waves"])
@pytest.mark.parametrize("width", E.LN_WIDTHS)
def test_layer_norm_backward_against_float64(native, width, key):
    _ln_case(native, _ln_rows(key), width, "normal")


@pytest.mark.parametrize("key", ["few", "waves"])
@pytest.mark.parametrize("width", E.LN_HARD_WIDTHS)
@pytest.mark.parametrize("kind", ["offset", "constant"])
def test_layer_norm_backward_on_offset_and_constant_rows(native, kind, width, key):
    _ln_case(native, _ln_rows(key), width, kind)
