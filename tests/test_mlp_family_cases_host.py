"""Host check of the fused-MLP family cases (tests/mlp_family_cases.py): plain fp32 arithmetic on the CPU meets the bars the
GPU tests hold the kernels to, at the row counts of an MI355X (256 CUs).  The kernels' own error is never the yardstick."""
import pytest
import torch

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
