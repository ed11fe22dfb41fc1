"""GPU: the split-K first Linear K16 (csrc/wide_linear.hip) against the float64 formulas of tests/image_mlp_cases.py over its table
of cases, for ReLU, one smooth activation (GELU) and Identity.

Bounds are the project's own: forward ``1e-5 * max(1, max|ref|)`` (test_gpu_readout_batched.py), gradients ``2e-5 + 1e-4 * max|ref|``
per tensor (test_gpu_ragged_batch_capture.py).  The measured worst errors are printed (``pytest -s``) and recorded in DESIGN K16."""
import functools

import pytest
import torch

from graphnet_classifier_amd import native
from tests import image_mlp_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACTIVATIONS = ["ReLU", "GELU", "Identity"]


@functools.lru_cache(maxsize=None)
def _case(case):
    """(x, W0, b0) float32 on the host and the float64 pre-activation z0 - computed once per case, never modified."""
    w, b, *_ = C.params64(C.reference_mlp(case))
    x = C.inputs(case)
    z0 = x.double() @ w[0].t() + b[0]
    return x, w[0].float(), b[0].float(), z0


@functools.lru_cache(maxsize=None)
def _reference(case, activation):
    x, w0, b0, z0 = _case(case)
    da = C.cotangent(case, width=w0.size(0))
    dz = da.double() * C.act_grad(z0, activation)
    return C.act(z0, activation), da, dz.t() @ x.double(), dz.sum(dim=0)


def _fwd_bound(ref):
    return 1e-5 * max(1.0, float(ref.abs().max()))


def _grad_bound(ref):
    return 2e-5 + 1e-4 * float(ref.abs().max())


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max())


@pytest.mark.parametrize("activation", ACTIVATIONS)
@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_forward_and_backward_equal_formulas(case, activation):
    x, w0, b0, z0 = _case(case)
    a_ref, da, dw_ref, db_ref = _reference(case, activation)
    xd, wd, bd = x.to(DEV), w0.to(DEV), b0.to(DEV)
    relu = activation == "ReLU"
    a0, zd = native.wide_linear_forward(xd, wd, bd, activation, want_z=not relu)
    assert a0.shape == a_ref.shape and (zd is None) == relu
    e_a = _err(a0, a_ref)
    e_z = _err(zd, z0) if zd is not None else 0.0
    dw, db = native.wide_linear_backward(da.to(DEV), a0 if relu else zd, xd, activation)
    e_w, e_b = _err(dw, dw_ref), _err(db, db_ref)
    print(f"\nK16 {C.case_id(case)} {activation}: a0 {e_a:.2e} (bound {_fwd_bound(a_ref):.2e}) z0 {e_z:.2e} "
          f"dW0 {e_w:.2e} (bound {_grad_bound(dw_ref):.2e}) db0 {e_b:.2e} (bound {_grad_bound(db_ref):.2e})")
    assert e_a <= _fwd_bound(a_ref)
    assert e_z <= _fwd_bound(z0)
    assert dw.shape == dw_ref.shape and e_w <= _grad_bound(dw_ref)
    assert e_b <= _grad_bound(db_ref)
    if relu:  # with the margin of the cases no unit may differ from the float64 model in being on or off
        assert torch.equal(a0.cpu() > 0, a_ref > 0)


@pytest.mark.parametrize("activation", ["ReLU", "GELU"])
@pytest.mark.parametrize("case", [(5, 1083, 40, 2), (33, 3072, 256, 2), (8, 49152, 128, 2)], ids=C.case_id)
def test_two_calls_are_bitwise_equal(case, activation):
    x, w0, b0, _ = _case(case)
    da = _reference(case, activation)[1].to(DEV)
    xd, wd, bd = x.to(DEV), w0.to(DEV), b0.to(DEV)
    runs = []
    for _ in range(2):
        a0, z0 = native.wide_linear_forward(xd, wd, bd, activation, want_z=True)
        dw, db = native.wide_linear_backward(da, a0 if activation == "ReLU" else z0, xd, activation)
        runs.append((a0, z0, dw, db))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("case", [(5, 1083, 40, 2), (17, 3072, 128, 2)], ids=C.case_id)
def test_views_with_unaligned_base_and_wider_pitch(case):
    """W0 as a column-offset view of a wider matrix (base not 16-B aligned, pitch K + 3), x with ld > K, the gradient of the
    output and a0 as column views: the same bits as the contiguous call."""
    x, w0, b0, _ = _case(case)
    rows, K, H = case[0], case[1], case[2]
    da = _reference(case, "ReLU")[1].to(DEV)
    xd, wd, bd = x.to(DEV), w0.to(DEV), b0.to(DEV)
    a_want, _ = native.wide_linear_forward(xd, wd, bd, "ReLU")
    dw_want, db_want = native.wide_linear_backward(da, a_want, xd, "ReLU")
    wide_w = torch.full((H, K + 3), 7.0, device=DEV)
    wide_w[:, 1:K + 1] = wd
    wide_x = torch.full((rows, K + 5), -3.0, device=DEV)
    wide_x[:, :K] = xd
    wv, xv = wide_w[:, 1:K + 1], wide_x[:, :K]
    assert wv.data_ptr() % 16 != 0 and wv.stride(0) == K + 3 and xv.stride(0) == K + 5
    a0, _ = native.wide_linear_forward(xv, wv, bd, "ReLU")
    assert torch.equal(a0, a_want)
    wide_g = torch.full((rows, H + 2), 9.0, device=DEV)
    wide_g[:, 1:H + 1] = da
    wide_a = torch.full((rows, H + 1), 5.0, device=DEV)
    wide_a[:, :H] = a0
    dw, db = native.wide_linear_backward(wide_g[:, 1:H + 1], wide_a[:, :H], xv, "ReLU")
    assert torch.equal(dw, dw_want) and torch.equal(db, db_want)


def test_nan_in_x_reaches_the_output_under_relu():
    case = (17, 3072, 128, 2)
    x, w0, b0, _ = _case(case)
    xd = x.to(DEV).clone()
    xd[3, 2000] = float("nan")
    a0, _ = native.wide_linear_forward(xd, w0.to(DEV), b0.to(DEV), "ReLU")
    assert bool(torch.isnan(a0[3]).all())
    assert not bool(torch.isnan(a0[:3]).any()) and not bool(torch.isnan(a0[4:]).any())


def test_no_bias_and_rejected_shapes():
    case = (8, 1200, 128, 2)
    x, w0, b0, z0 = _case(case)
    a0, _ = native.wide_linear_forward(x.to(DEV), w0.to(DEV), None, "Identity")
    ref = z0 - b0.double()
    assert _err(a0, ref) <= _fwd_bound(ref)
    with pytest.raises(RuntimeError):
        native.wide_linear_forward(x.to(DEV)[:, :1000], w0.to(DEV)[:, :1000], None)  # K < 1024
