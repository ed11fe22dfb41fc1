"""GPU tests of the batch-norm kernels (K14, csrc/batchnorm.hip) and of the norm_type='BatchNorm1d' route through them:
statistics on ill-conditioned columns, apply + residual, backward, running statistics, the eval-mode fold, the module routing
(no call of ``torch.nn.functional.batch_norm`` is left), the reference's golden vectors and a captured training step.
References: tests/batchnorm_cases.py (float64, pinned on the host by tests/test_batchnorm_host.py)."""
import ast
import functools

import numpy as np
import pytest
import torch

from tests import batchnorm_cases as B
from tests._util import load_golden, max_abs, sub_state_dict, t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def native():
    from graphnet_classifier_amd import native
    native.load_library()
    torch.cuda.set_device(0)
    return native


@functools.lru_cache(maxsize=None)
def _device_rows(width: int):
    """(smallest row count with two partial rows, a row count that reaches the grid cap with a ragged last range)."""
    from graphnet_classifier_amd import native
    with torch.cuda.device(0):
        two = next(r for r in range(2, 1 << 14) if native.bn_partials(r, width) == 2)
        tile = two - 1
        cap = max(native.bn_partials(tile << j, width) for j in range(0, 16))
        full = (cap - 1) * tile + 1
        assert native.bn_partials(two - 1, width) == 1 and native.bn_partials(full, width) == cap
        assert native.bn_partials(full + tile, width) < cap  # beyond the cap a workgroup owns several tiles
    return two, full


def _rows(width):
    from graphnet_classifier_amd import native
    assert B.SMALL_EDGE == (native.bn_small_max_rows(), native.bn_small_max_rows() + 1)
    return B.ROWS + B.SMALL_EDGE + _device_rows(width)


def _wide(x: torch.Tensor, pad: int) -> torch.Tensor:
    """The same values as a column slice of a wider device table (ld > C)."""
    big = torch.full((x.size(0), x.size(1) + pad), float("nan"), device=DEV)
    big[:, :x.size(1)] = x.to(DEV)
    return big[:, :x.size(1)]


def _check_stats(native, d, z):
    mean, invstd = native.bn_stats(z, B.EPS)
    mean2, invstd2 = native.bn_stats(z, B.EPS)
    assert torch.equal(mean, mean2) and torch.equal(invstd, invstd2), "not bitwise reproducible"
    var = 1.0 / invstd.double().cpu() ** 2 - B.EPS
    mean_err = (mean.double().cpu() - d["mean"]).abs() / d["colmax"]
    var_err = (var - d["var"]).abs() / d["var"]
    print(f"rows {z.size(0)} width {z.size(1)}: mean err / max|z| {float(mean_err.max()):.2e}, relative var err {float(var_err.max()):.2e}")
    assert float(mean_err.max()) <= 1e-6 and float(var_err.max()) <= 1e-4
    if z.size(0) <= native.bn_small_max_rows():  # the one-launch kernel forms its own statistics: the same bounds
        ones, zeros = torch.ones(z.size(1), device=DEV), torch.zeros(z.size(1), device=DEV)
        _, m1, i1 = native.bn_forward(z, ones, zeros, eps=B.EPS)
        _, m2, i2 = native.bn_forward(z, ones, zeros, eps=B.EPS)
        assert torch.equal(m1, m2) and torch.equal(i1, i2), "not bitwise reproducible"
        mean_err = (m1.double().cpu() - d["mean"]).abs() / d["colmax"]
        var_err = (1.0 / i1.double().cpu() ** 2 - B.EPS - d["var"]).abs() / d["var"]
        print(f"  one launch: mean err / max|z| {float(mean_err.max()):.2e}, relative var err {float(var_err.max()):.2e}")
        assert float(mean_err.max()) <= 1e-6 and float(var_err.max()) <= 1e-4


@pytest.mark.parametrize("width", B.WIDTHS)
def test_statistics_of_ill_conditioned_columns(native, width):
    for rows in _rows(width):
        d = B.ill_conditioned(rows, width)
        _check_stats(native, d, d["z"].to(DEV))


@pytest.mark.parametrize("rows", [65, 4099])  # the one-launch kernels and the streaming ones
@pytest.mark.parametrize("width,pad", [(20, 4), (5, 2), (64, 64)])
def test_statistics_and_apply_with_a_row_stride_above_the_width(native, width, pad, rows):
    d = B.ill_conditioned(rows, width)
    _check_stats(native, d, _wide(d["z"], pad))
    w = B.well_conditioned(rows, width)
    z, res, g = _wide(w["z"], pad), _wide(w["residual"], pad), _wide(w["grad_out"], pad)
    out, mean, invstd = native.bn_forward(z, w["gamma"].to(DEV), w["beta"].to(DEV), res, eps=B.EPS)
    assert max_abs(out.cpu(), w["out"]) <= B.bound(w["out"])
    dz, dgamma, dbeta = native.bn_backward(g, z, mean, invstd, w["gamma"].to(DEV))
    for got, name in ((dz, "dz"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        assert max_abs(got.cpu(), w[name]) <= B.bound(w[name]), name
    assert bool(torch.isnan(z._base[:, width:]).all()), "wrote outside the table's columns"


@pytest.mark.parametrize("width", B.WIDTHS)
def test_forward_backward_and_running_statistics(native, width):
    from graphnet_classifier_amd import functional as Fn
    for rows in _rows(width):
        w = B.well_conditioned(rows, width)
        z = w["z"].to(DEV).requires_grad_(True)
        gamma, beta = w["gamma"].to(DEV).requires_grad_(True), w["beta"].to(DEV).requires_grad_(True)
        res = w["residual"].to(DEV).requires_grad_(True)
        rm, rv = w["running_mean"].to(DEV), w["running_var"].to(DEV)
        out = Fn.batch_norm_rows(z, gamma, beta, res, rm, rv, B.MOMENTUM, B.EPS, True)
        grad = w["grad_out"].to(DEV)
        dz, dgamma, dbeta, dres = torch.autograd.grad(out, [z, gamma, beta, res], grad)
        errs = {"out": (out.detach(), w["out"]), "dz": (dz, w["dz"]), "dgamma": (dgamma, w["dgamma"]), "dbeta": (dbeta, w["dbeta"]),
                "running_mean": (rm, w["new_running_mean"]), "running_var": (rv, w["new_running_var"])}
        for name, (got, ref) in errs.items():
            err = max_abs(got.cpu(), ref)
            print(f"rows {rows} width {width} {name}: {err:.2e} (bound {B.bound(ref):.2e})")
            assert err <= B.bound(ref), (rows, name)
        assert dres.data_ptr() == grad.data_ptr(), "the residual's gradient is grad_out itself, not a copy"
        # no residual, nothing wanted: the same numbers, and the in-place form writes them over z
        with torch.no_grad():
            rm2, rv2 = w["running_mean"].to(DEV), w["running_var"].to(DEV)
            zc = w["z"].to(DEV)
            plain = Fn.batch_norm_rows(zc, gamma, beta, None, rm2, rv2, B.MOMENTUM, B.EPS, True, inplace=True)
            assert plain.data_ptr() == zc.data_ptr() and max_abs(plain.cpu(), w["out_plain"]) <= B.bound(w["out_plain"])
            assert torch.equal(rm2, rm) and torch.equal(rv2, rv), "not bitwise reproducible"
        # backward twice: bitwise equal
        again = torch.autograd.grad(Fn.batch_norm_rows(z, gamma, beta, res, rm2, rv2, B.MOMENTUM, B.EPS, True), [z, gamma, beta], grad)
        assert all(torch.equal(a, b) for a, b in zip(again, (dz, dgamma, dbeta)))


@pytest.mark.parametrize("width", [130, 256])
def test_apply_and_backward_beyond_two_passes_of_their_capped_grid(native, width):
    """gnc_bn_apply_f32 and gnc_bn_backward_dz_f32 run at most 8 workgroups per CU; a workgroup of 256 / lanes row slots takes
    the rows r, r + s, r + 2 s, r + 3 s (s = the grid's slots) per trip.  The largest row count of ``_rows`` (the reducing
    kernels' cap) stays inside ONE such trip.  Here: two full trips and 83 rows on a third (a ragged last workgroup), at 64
    lanes per row with vector (256) and scalar (130) rows, against the same float64 references and bound."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_per_trip = 4 * (256 // 64)  # of one workgroup
    rows = 2 * 8 * cus * rows_per_trip + 5 * rows_per_trip + 3
    assert rows > 2 * 8 * cus * rows_per_trip and max(_rows(width)) <= 8 * cus * rows_per_trip
    w = B.well_conditioned.__wrapped__(rows, width)  # (not kept in the case cache: 67 MB a tensor)
    z, res, g = w["z"].to(DEV), w["residual"].to(DEV), w["grad_out"].to(DEV)
    out, mean, invstd = native.bn_forward(z, w["gamma"].to(DEV), w["beta"].to(DEV), res, eps=B.EPS)
    dz, dgamma, dbeta = native.bn_backward(g, z, mean, invstd, w["gamma"].to(DEV))
    for got, name in ((out, "out"), (dz, "dz"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        err = max_abs(got.cpu(), w[name])
        print(f"rows {rows} width {width} {name}: {err:.2e} (bound {B.bound(w[name]):.2e})")
        assert err <= B.bound(w[name]), name


def test_one_row_is_refused_like_pytorch_and_batches_are_counted(native):
    from graphnet_classifier_amd.MLP import MLP
    m = MLP(12, 20, hidden_dim=32, norm_type="BatchNorm1d").train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.randn(1, 12, device=DEV))
    assert int(m.model[-1].num_batches_tracked) == 0
    m(torch.randn(9, 12, device=DEV))
    m(torch.randn(2, 12, device=DEV))
    assert int(m.model[-1].num_batches_tracked) == 2
    m.eval()(torch.randn(1, 12, device=DEV))  # eval mode normalises row by row: one row is fine
    assert int(m.model[-1].num_batches_tracked) == 2


def _cpu_twin(m):
    """The same Sequential in PyTorch on the CPU."""
    twin = torch.nn.Sequential(*[type(l)(**({"in_features": l.in_features, "out_features": l.out_features} if isinstance(l, torch.nn.Linear)
                                            else {"num_features": l.num_features} if isinstance(l, torch.nn.BatchNorm1d) else {}))
                                 for l in m.model])
    twin.load_state_dict({k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()})
    return twin


def test_module_route_never_calls_the_library_batch_norm(native, monkeypatch):
    from graphnet_classifier_amd.MLP import MLP
    torch.manual_seed(5)
    m = MLP(12, 20, hidden_dim=32, norm_type="BatchNorm1d")
    with torch.no_grad():
        m.model[-1].weight.uniform_(0.5, 1.5); m.model[-1].bias.uniform_(-0.5, 0.5)
    twin = _cpu_twin(m).train()
    x, res, wgt = torch.randn(50, 12), torch.randn(50, 20), torch.randn(50, 20)

    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.batch_norm was called: the norm left the library")
    ref = twin(x) + res          # PyTorch on the CPU first: the patch below would stop it too
    twin64 = _cpu_twin(m).double().train()
    (twin64(x.double()) * wgt.double()).sum().backward()
    twin.eval()
    ref_eval = twin(x).detach() + res
    monkeypatch.setattr(torch.nn.functional, "batch_norm", refuse)
    m.train()
    xd, rd = x.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
    y = m.forward_segments([(xd, None)], residual=rd)
    (y * wgt.to(DEV)).sum().backward()
    assert max_abs(y.detach().cpu(), ref.detach()) <= 2e-5
    # gradients against float64.  One bound for the module, from its largest gradient: the Linear bias in front of the norm has a
    # true gradient of 0, and its fp32 value is the rounding of column sums whose terms are as large as its neighbours' terms
    # (this loss weights every output with an N(0, 1) number, so they are ~1000 times those of a mean-reduced loss)
    grad_bound = B.bound(torch.cat([q.grad.flatten() for q in twin64.parameters()]))
    for (k, p), q in zip(m.model.named_parameters(), twin64.parameters()):
        assert max_abs(p.grad.cpu(), q.grad) <= grad_bound, k
    assert max_abs(rd.grad.cpu(), wgt) == 0 and float(xd.grad.abs().max()) > 0
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert max_abs(getattr(m.model[-1], k).cpu(), getattr(twin[-1], k)) <= 1e-6, k
    m.eval()
    with torch.no_grad():
        y_eval = m.forward_segments([(x.to(DEV), None)], residual=res.to(DEV))
    assert max_abs(y_eval.cpu(), ref_eval) <= 2e-5


def test_fold_follows_the_live_weights_and_running_statistics(native):
    from graphnet_classifier_amd.MLP import MLP
    torch.manual_seed(6)
    m = MLP(12, 20, hidden_dim=32, norm_type="BatchNorm1d")
    bn = m.model[-1]
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-1, 1); bn.running_var.uniform_(0.5, 2.0)
    m.eval()
    x = torch.randn(300, 12)
    with torch.no_grad():
        assert max_abs(m(x.to(DEV)).cpu(), _cpu_twin(m).eval()(x)) <= 2e-5
        first = m(x.to(DEV)).clone()
        m.model[4].weight.mul_(1.5)          # in place: no new tensor, no version the module could look at through .data
        bn.running_var.data.mul_(3.0)
        second = m(x.to(DEV))
        assert max_abs(second.cpu(), _cpu_twin(m).eval()(x)) <= 2e-5
        assert max_abs(first, second) > 1e-2


def test_edge_feature_prologue_serves_an_eval_mode_batchnorm_encoder(native):
    from graphnet_classifier_amd.MLP import MLP
    torch.manual_seed(7)
    enc = MLP(3, 64, hidden_dim=64, norm_type="BatchNorm1d")
    with torch.no_grad():
        enc.model[-1].running_mean.uniform_(-1, 1); enc.model[-1].running_var.uniform_(0.5, 2.0)
    rng = np.random.default_rng(7)
    n, e = 5000, 300000
    pos = torch.from_numpy((rng.random((n, 2)) * 8).astype(np.float32)).to(DEV)
    src = torch.from_numpy(rng.integers(0, n, size=e).astype(np.int32)).to(DEV)
    dst = torch.from_numpy(rng.integers(0, n, size=e).astype(np.int32)).to(DEV)
    with torch.no_grad():
        assert enc.train().forward_edge_features(pos, src, dst) is None  # batch statistics need the rows
        got = enc.eval().forward_edge_features(pos, src, dst)
        assert got is not None, "an eval-mode BatchNorm encoder folds into the launch that carries the prologue"
        stored = enc.forward_segments([(native.edge_features(pos, src, dst), None)])
    assert max_abs(got, stored) <= 1e-5


@pytest.mark.parametrize("tag", ["w16", "w64"])
def test_reference_golden_g11(native, tag):
    from graphnet_classifier_amd import GNN
    g = load_golden("g11_batchnorm.npz")
    kw = ast.literal_eval(bytes(g[f"{tag}/kwargs_json"]).decode())
    x, pos, ei, label = (t(g[f"{tag}/{k}"]) for k in ("x", "pos", "edge_index", "label"))
    m = GNN.CombinedModel(GNN.GraphNet(**kw), num_nodes=x.size(0), classes=2)
    m.load_state_dict(sub_state_dict(g, f"{tag}/sd/"), strict=True)
    kept = {}
    # the per-node GraphNet output is what the read-out is called with (flattened)
    m.classifier.register_forward_pre_hook(lambda mod, inp: kept.__setitem__("y", inp[0].detach().clone().view(x.size(0), -1)))
    m.train()
    logits = m((x.to(DEV), pos.to(DEV), ei))
    loss = torch.nn.CrossEntropyLoss()(logits, label.to(DEV))
    loss.backward()
    assert max_abs(kept["y"].cpu(), t(g[f"{tag}/train_y"])) <= 1e-5 and max_abs(logits.detach().cpu(), t(g[f"{tag}/train_logits"])) <= 1e-5
    assert max_abs(loss.detach().cpu(), t(g[f"{tag}/loss"])) <= 1e-6
    for k, p in m.named_parameters():
        ref = t(g[f"{tag}/grad/{k}"])
        assert p.grad is not None and max_abs(p.grad.cpu(), ref) <= B.bound(ref), k
    buffers = dict(m.named_buffers())
    after = sub_state_dict(g, f"{tag}/after/")
    assert set(after) <= set(buffers) and after
    for k, ref in after.items():
        assert max_abs(buffers[k].cpu(), ref) <= 1e-6, k
    m.eval()
    with torch.no_grad():
        eval_logits = m((x.to(DEV), pos.to(DEV), ei))
    assert max_abs(kept["y"].cpu(), t(g[f"{tag}/eval_y"])) <= 1e-5 and max_abs(eval_logits.cpu(), t(g[f"{tag}/eval_logits"])) <= 1e-5


def test_captured_training_steps_equal_eager_steps_bitwise(native):
    """Three steps through the fixed-topology CapturedTrainStep and three eager steps from the same start: every state_dict
    entry (the BatchNorm buffers included) and the loss sum are bitwise equal - the K14 launches sit inside the captured graph
    (no memset node, no host value) and are reproducible."""
    from graphnet_classifier_amd import GNN
    from graphnet_classifier_amd.train import CapturedTrainStep, FlatParameters, FusedAdam
    g = load_golden("g8_training_run.npz")
    kw = dict(ast.literal_eval(bytes(g["kwargs_json"]).decode()), norm_type="BatchNorm1d")
    pos, ei = t(g["pos"]), t(g["edge_index"])
    ds = [((t(g[f"x{k}"]), pos, ei), torch.tensor(int(g["labels"][k]))) for k in range(2)]
    crit = torch.nn.CrossEntropyLoss()
    torch.manual_seed(0)
    start = {k: v.detach().clone() for k, v in GNN.CombinedModel(GNN.GraphNet(**kw), num_nodes=64, classes=2).state_dict().items()}
    order = (ds[0], ds[1], ds[0])
    finals = {}
    for mode in ("captured", "eager"):
        m = GNN.CombinedModel(GNN.GraphNet(**kw), num_nodes=64, classes=2)
        m.load_state_dict(start, strict=True)
        m.train()
        opt = FusedAdam(FlatParameters(m))
        loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)
        if mode == "captured":
            step = CapturedTrainStep(m, opt, crit, *ds[0], loss_sum)
            for s, l in order:
                step(s, l)
        else:
            for s, l in order:
                loss = crit(m((s[0].to(DEV), s[1].to(DEV), s[2])), l.to(DEV))
                opt.zero_grad(); loss.backward(); opt.step()
                loss_sum += loss.detach().double()
        torch.cuda.synchronize()
        finals[mode] = ({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, float(loss_sum))
    assert finals["captured"][1] == finals["eager"][1] and np.isfinite(finals["eager"][1])
    assert any(k.endswith("num_batches_tracked") and int(v) == 3 for k, v in finals["eager"][0].items())
    for k, v in finals["eager"][0].items():
        assert torch.equal(finals["captured"][0][k], v), k
    assert all(not torch.equal(v, start[k].cpu()) for k, v in finals["eager"][0].items() if "running_" in k)
