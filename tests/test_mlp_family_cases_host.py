"""Host check of the fused-MLP family cases (tests/mlp_family_cases.py): plain fp32 arithmetic on the CPU meets the bars the
GPU tests hold the kernels to, at the row counts of an MI355X (256 CUs).  The kernels' own error is never the yardstick."""
import pytest
import torch

from tests import elementwise_cases as E
from tests import mlp_family_cases as M

ROWS = M.MI355X_ROWS


def test_row_counts_of_an_mi355x():
    assert (ROWS["first"], ROWS["loop"], ROWS["bwd"]) == (32769, 65829, 16421)


@pytest.mark.parametrize("name", [c.name for c in M.CASES])
def test_forward_cases_are_within_their_bar_in_fp32(name):
    for key in M.forward_rows(M.BY_NAME[name]):
        c = M.build(name, ROWS[key])
        with torch.no_grad():
            out, acts, _, _ = M.evaluate(c, torch.float32)
        assert float((out.double() - c["out"]).abs().max()) < c["bar"], key
        for a, want in zip(acts, c["acts"]):
            assert float((a.double() - want).abs().max()) < M.TOL * max(1.0, float(want.abs().max())), key


@pytest.mark.parametrize("name,key", [(c.name, k) for c, keys in M.BWD_CASES for k in keys])
def test_backward_cases_mark_at_most_one_percent_of_their_rows(name, key):
    c = M.build(name, ROWS[key])
    marked = torch.zeros(c["rows"], dtype=torch.bool)
    for z in c["pre"]:
        marked |= (z.abs() < M.KINK).any(dim=1)
    assert float(marked.float().mean()) <= M.KINK_SHARE


# One backward case per width class at rows_loop: the sums over 65,829 rows (weight gradients, LayerNorm sums) of fp32 CPU
# autograd against float64.  Measured here: dW / db 5.5e-7 of max(1, max|g|) (bar 1e-4: stays), dz[0] / dx 6.9e-6 (bar 2e-5:
# stays), LayerNorm sums 2.56e-3 / 1.66e-3 / 1.52e-3: the 1e-3 bar is NOT met by fp32 arithmetic at this row count, so the
# GPU tests use 3 x 2.56e-3 there (mlp_family_cases.LN_SUM_BAR_LOOP); at 16,421 rows fp32 is 7e-4 off at most and 1e-3 stays.
@pytest.mark.parametrize("name", ["bwd_edge_wsplit_128", "bwd_node_48", "bwd_plain_200"])
def test_fp32_autograd_meets_the_gradient_bars_at_rows_loop(name):
    c = M.build_backward(name, ROWS["loop"])
    assert c["marked_share"] <= M.KINK_SHARE
    got = M.autograd(c, torch.float32, c["grad_out"])
    want = c["grads"]
    worst = 0.0
    for g, w in zip(got["dw"] + got["db"], want["dw"] + want["db"]):
        rel = float((g.double() - w).abs().max()) / max(1.0, float(w.abs().max()))
        worst = max(worst, rel)
        assert rel < M.DW_BAR
    ln = max(float((got[k].double() - want[k]).abs().max()) for k in ("dgamma", "dbeta"))
    print(f"{name}: fp32-CPU dW/db error {worst:.2e} (bar {M.DW_BAR:.0e}), LayerNorm sums {ln:.2e} (bar {M.LN_SUM_BAR_LOOP:.1e})")
    assert ln < M.LN_SUM_BAR_LOOP  # (the summation order, and with it this figure, depends on the host's thread count)
    assert float((got["dz0"].double() - want["dz0"]).abs().max()) < M.DX_BAR
    assert float((got["dx"].double() - want["dx"]).abs().max()) < M.DX_BAR


# ------------------------------------------------------------------------------------------------ the generic kernel's cases
CU, SMALL_BATCH = 256, 128 * 256


def test_generic_row_counts_of_an_mi355x():
    assert [M.generic_loop_rows(CU, wt) for wt in (1, 2, 4, 8)] == [98469, 98469, 65701, 32933]
    assert M.generic_loop_rows(CU, 8, layers=4) == 32933 and M.generic_loop_rows(CU, 4, layers=4) == 65701
    assert M.MI355X_ROWS["bwd"] == 64 * CU + 37


def test_generic_cases_cover_every_instance_activation_and_padded_width():
    non_relu = [c for c in M.GENERIC_CASES if c.activation != "ReLU"]
    instances = {(1, 1), (2, 2), (2, 1), (4, 4), (4, 1), (8, 8), (8, 1)}
    assert {M.generic_tiles(c) for c in non_relu} == instances  # at ``small`` ...
    assert {M.generic_tiles(M.GENERIC_BY_NAME[n]) for n in M.GENERIC_LOOP} == instances  # ... and with more tiles than the grid
    assert all(M.GENERIC_BY_NAME[n].activation != "ReLU" for n in M.GENERIC_LOOP)
    for cases in (non_relu, M.GENERIC_BWD_CASES):
        for widths in M.GENERIC_WIDTH_CLASSES:
            if any(c.dims[0] in widths for c in cases):
                assert {c.activation for c in cases if c.dims[0] in widths} == set(M.ACT_PARAM), widths
        for w in M.PADDED_WIDTHS:
            assert {"Sigmoid", "GELU"} <= {c.activation for c in cases if c.dims[0] == w}, w
    assert {c.dims[0] for c in M.GENERIC_BWD_CASES} == {20, 48, 100, 128, 200}
    assert any(c.sliced for c in non_relu) and any(c.nobias and not c.shared for c in non_relu)
    assert {len(c.dims) for c in non_relu} >= {2, 3, 4}
    assert all(M.ACT_PARAM[c.activation] == c.act_param for c in non_relu)


@pytest.mark.parametrize("name", [c.name for c in M.GENERIC_CASES])
def test_generic_forward_cases_are_within_their_bar_in_fp32(name):
    case = M.GENERIC_BY_NAME[name]
    for key, rows in M.generic_rows(case, SMALL_BATCH, CU).items():
        c = M.build(name, rows)
        with torch.no_grad():
            out = M.evaluate(c, torch.float32)[0]
        assert float((out.double() - c["out"]).abs().max()) < c["bar"], key


# One backward case per width class at both row counts, the gathered shape among them.  Measured here (fp32 CPU autograd against
# float64, worst of 777 and 16,421 rows): dx 4.0e-6 (bar 2e-5), gathered table 3.8e-7 and dW / db 7.9e-7 of max(1, max|g|) (bar
# 1e-4), LayerNorm sums 4.5e-4 (bar 1e-3): every bar is met by fp32 arithmetic.
@pytest.mark.parametrize("key", M.GENERIC_BWD_KEYS)
@pytest.mark.parametrize("name", ["gbwd_concat_edge_20_Tanh", "gbwd_node_48_Sigmoid", "gbwd_concat_edge_128_Sigmoid", "gbwd_plain_200_ELU"])
def test_fp32_autograd_meets_the_gradient_bars_of_the_generic_backward(name, key):
    c = M.build_backward(name, M.MI355X_ROWS[key])
    assert c["marked_share"] <= M.KINK_SHARE
    case, want = c["case"], c["grads"]
    got = M.autograd(c, torch.float32, c["grad_out"])
    err = lambda g, w: float((g.double() - w).abs().max())  # noqa: E731
    worst = {"dx": 0.0, "table": 0.0, "dw": 0.0}
    for g, w, (_, ix, _) in zip(M.table_gradients(c, got, c["grad_out"]), M.table_gradients(c, want, c["grad_out"]), case.segs):
        if ix is None:
            worst["dx"] = max(worst["dx"], err(g, w))
        else:
            worst["table"] = max(worst["table"], err(g, w) / max(1.0, float(w.abs().max())))
    for g, w in zip(got["dw"] + got["db"], want["dw"] + want["db"]):
        if w is not None:
            worst["dw"] = max(worst["dw"], err(g, w) / max(1.0, float(w.abs().max())))
    worst["ln"] = max(err(got[k], want[k]) for k in ("dgamma", "dbeta")) if case.ln else 0.0
    print(f"{name}/{key}: fp32-CPU " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["dx"] < M.DX_BAR and worst["table"] < M.DW_BAR and worst["dw"] < M.DW_BAR and worst["ln"] < M.LN_SUM_BAR


# ------------------------------------------------------------------------------------------------ the row-wise kernels' formulas
@pytest.mark.parametrize("name,param", E.ACTS)
def test_fp32_formulas_of_the_activations_are_within_their_bars(name, param):
    x = E.table()
    ref_a, ref_d = E.reference(x, name, param)
    a, d = E.fp32_formulas(x, name, param)
    for what, got, ref in (("forward", a, ref_a), ("derivative", d, ref_d)):
        e = E.errors(got, ref, x)
        print(f"{name} {what}: fp32-CPU abs {e['abs']:.2e} (bar {E.ABS_BAR:.0e}), rel {e['rel']:.2e} (bar {E.REL_BAR:.0e})")
        assert e["finite"] and e["abs"] <= E.ABS_BAR and e["rel"] <= E.REL_BAR


def test_elu_by_expf_minus_one_misses_the_relative_bar():
    """The form both ELU forwards had: fine absolutely, every digit lost near 0 (the reason they use expm1f)."""
    x = E.table()
    ref = E.reference(x, "ELU", 1.0)[0]
    e = E.errors(torch.where(x > 0, x, torch.exp(x) - 1.0), ref, x)
    assert e["abs"] <= E.ABS_BAR and e["rel"] > 0.5


@pytest.mark.parametrize("kind,widths", [("normal", E.LN_WIDTHS), ("offset", E.LN_HARD_WIDTHS), ("constant", E.LN_HARD_WIDTHS)])
def test_fp32_layer_norm_backward_is_within_its_bars(kind, widths):
    worst = [0.0, 0.0]
    for width in widths:
        for rows in (1, 37, 64 * CU + 37):
            y, gamma, g = E.ln_inputs(rows, width, kind)
            ref_dy, ref_yh = E.ln_reference(y, gamma, g)
            dy, yh = E.ln_fp32(y, gamma, g)
            bar_dy, bar_yh = E.ln_bars(kind, ref_yh)
            e_dy, e_yh = float((dy.double() - ref_dy).abs().max()), float((yh.double() - ref_yh).abs().max())
            worst = [max(worst[0], e_dy), max(worst[1], e_yh)]
            assert e_dy < bar_dy and e_yh < bar_yh, (width, rows)
    print(f"{kind}: fp32-CPU dy {worst[0]:.2e}, y_hat {worst[1]:.2e}")
