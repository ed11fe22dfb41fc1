"""The fused MLP (forward K4, backward K8) at the row counts that reach its throughput kernels: every shape sweep of
tests/mlp_family_cases.py runs above the small-batch limit (the first row count the 32-row / 16-row streaming kernels see)
and with more tiles than a persistent grid has waves, each launch against the float64 definition of the same operation.
Row counts come from the device (small-batch limit, CU count), never from a constant.

The split class of the weights-resident kernel (3-way bf16 split) is additionally held against the exact fp32 path of the
same launch (GNC_MLP_F32_EXACT=1, read once per process: one child process per class)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import mlp_family_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from graphnet_classifier_amd import native as n
    n.load_library()
    return n


@functools.lru_cache(maxsize=None)
def _rows() -> dict:
    from graphnet_classifier_amd import native as n
    small = int(n.load_library().gnc_mlp_small_batch_max_rows())
    return M.derived_rows(small, torch.cuda.get_device_properties(0).multi_processor_count)


def _upload(c):
    case = c["case"]
    tabs = [M.to_device(op, DEV) for op in c["tables"]]
    idx = {k: v.to(DEV) for k, v in c["index"].items()}
    return dict(tabs=tabs, idx=idx, segs=[(t, idx[ix] if ix else None) for t, (_, ix, _) in zip(tabs, case.segs)],
                ws=[M.to_device(w, DEV) for w in c["ws"]], bs=[b.to(DEV) if b is not None else None for b in c["bs"]],
                ln=(c["ln"][0].to(DEV), c["ln"][1].to(DEV), c["ln"][2]) if c["ln"] else None,
                residual=tabs[case.res] if case.res is not None else None, modes=case.modes if any(case.modes) else None,
                pos=c["pos"].to(DEV) if c["pos"] is not None else None)


def _forward(native, c, d, save=None):
    if c["case"].k6:  # the edge encoder with K6 as its prologue: the [rows, 3] table is never stored
        out = native.mlp_forward_edge_features(d["pos"], d["idx"]["src"], d["idx"]["dst"], d["ws"], d["bs"], ln=d["ln"])
        assert out is not None, "the weights-resident kernel should serve this shape"
        return out
    return native.mlp_forward(d["segs"], d["ws"], d["bs"], ln=d["ln"], residual=d["residual"], rows=c["rows"], modes=d["modes"],
                              save_act=save)


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


def _digest(t):
    return hashlib.sha1(t.cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the exact fp32 path
def _exact_child(family, path):
    """Runs in a fresh process with GNC_MLP_F32_EXACT=1: per case and row count of a split class the error of the exact fp32
    launch against float64 and a digest of its output bits."""
    from graphnet_classifier_amd import native
    native.load_library()
    res = {}
    for case in M.CASES:
        if case.family != family:
            continue
        for key in M.forward_rows(case):
            c = M.build(case.name, _rows()[key])
            out = _forward(native, c, _upload(c))
            res[f"{case.name}/{key}"] = [_err(out, c["out"]), _digest(out)]
    with open(path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def exact_runs(tmp_path_factory):
    done = {}

    def get(family):
        if family not in done:
            path = str(tmp_path_factory.mktemp("exact") / f"{family}.json")
            env = dict(os.environ, GNC_MLP_F32_EXACT="1")
            code = (f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_gpu_mlp_families as m; "
                    f"m._exact_child({family!r}, {path!r})")
            r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-3000:]
            with open(path) as f:
                done[family] = json.load(f)
        return done[family]

    return get


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name,key", [(c.name, k) for c in M.CASES for k in M.forward_rows(c)])
def test_forward_against_float64(native, exact_runs, name, key):
    c = M.build(name, _rows()[key])
    case, d = c["case"], _upload(c)
    if case.family == "stream":  # a later change of the small-batch limit fails here instead of moving the case silently
        assert not native.small_batch_kernel_serves(d["segs"], d["ws"], d["bs"], d["ln"], "ReLU", d["residual"], c["rows"], d["modes"])
    out = _forward(native, c, d)
    err = _err(out, c["out"])
    print(f"{name}/{key}: rows {c['rows']}, max-abs error vs float64 {err:.3e} (bar {c['bar']:.3e})")
    assert err < c["bar"]
    assert torch.equal(_forward(native, c, d), out)  # run-to-run determinism
    if len(case.dims) >= 2 and not case.k6:  # the training forward: same output bits, saved post-activations within the bar
        acts = []
        assert torch.equal(_forward(native, c, d, save=acts), out)
        assert len(acts) in (0, len(case.dims) - 1)
        for a, want in zip(acts, c["acts"]):
            assert _err(a, want) < M.TOL * max(1.0, float(want.abs().max()))
    if case.family in M.SPLIT_FAMILIES:
        err_exact, digest_exact = exact_runs(case.family)[f"{name}/{key}"]
        print(f"{name}/{key}: split {err:.3e}, fp32 exact {err_exact:.3e}")
        assert _digest(out) != digest_exact  # the split instance did run
        assert err <= 2.0 * err_exact


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("form", ["recompute", "saved"])
@pytest.mark.parametrize("name,key", [(c.name, k) for c, keys in M.BWD_CASES for k in keys])
def test_backward_against_float64_autograd(native, name, key, form):
    """dz[0], dx, the weight gradients and the LayerNorm sums of the K8 kernels against float64 autograd, recomputing and on the
    activations the forward of the same case saved.  Rows with a ReLU kink carry a zero output gradient (see the cases)."""
    c = M.build_backward(name, _rows()[key])
    assert c["marked_share"] <= M.KINK_SHARE
    case, d, want = c["case"], _upload(c), c["grads"]
    width = case.dims[0]
    gout = c["grad_out"].to(DEV)
    acts = []
    if form == "saved":
        _forward(native, c, d, save=acts)
    r = native.mlp_backward(d["segs"], d["ws"], d["bs"], d["ln"], gout, rows=c["rows"], modes=d["modes"], need_dx=True,
                            residual=d["residual"], saved_act=acts or None)
    if form == "recompute":
        assert not r["saved_act_used"]
    elif width > 32 and not name.startswith("bwd_decoder"):
        # 65..128: the persist kernel (128) / launch_bwd_stream<4, W, saved>; 129..256: the 16-row kernel; 33..64: the fused
        # data + weight-gradient kernel and the node processors' SAVED instance of the weights-resident data kernel
        assert len(acts) == 2 and r["saved_act_used"]
    else:  # one 32-column tile, and the decoders (above the small-batch limit no forward kernel with a narrow output saves):
        assert r["saved_act_used"] == bool(acts)  # a forward saves only what its backward reads
    if r["dz"][0] is not None:
        assert _err(r["dz"][0], want["dz0"]) < M.DX_BAR
    dx_ref = want["dx"].clone()
    if case.res is not None and not r["residual_folded"]:  # the kernel's dx then excludes the residual path
        c0 = sum(w for w, _, m in case.segs[:case.res] if m == M.SEG_MATMUL)
        dx_ref[:, c0:c0 + case.segs[case.res][0]] -= c["grad_out"].double()
    assert _err(r["dx"], dx_ref) < M.DX_BAR
    x_mm = None
    for l in range(len(case.dims)):
        if "dw" in r:
            dw, db = r["dw"][l], r["db"][l]
        else:
            if l == 0:
                x_mm = torch.cat([t for t, m in zip(d["tabs"], case.modes) if m == M.SEG_MATMUL], dim=1)
            dw, db = native.xty(r["dz"][l], x_mm if l == 0 else r["act"][l - 1])
        for got, ref in ((dw, want["dw"][l]), (db, want["db"][l])):
            assert _err(got, ref) < M.DW_BAR * max(1.0, float(ref.abs().max())), l
    if case.ln:
        dbeta, dgamma = r["ln_sums"] if r["ln_sums"] is not None else native.colsum_pair(gout, r["yhat"])
        bar = M.LN_SUM_BAR_LOOP if key == "loop" else M.LN_SUM_BAR
        e_g, e_b = _err(dgamma, want["dgamma"]), _err(dbeta, want["dbeta"])
        print(f"{name}/{key}/{form}: LayerNorm sums off by {e_g:.2e} / {e_b:.2e} (bar {bar:.1e})")
        assert e_g < bar and e_b < bar


# ------------------------------------------------------------------------------------------------ weight-gradient product
@pytest.mark.parametrize("m,k", [(64, 192), (128, 128), (200, 296)])
def test_xty_at_rows_loop(native, m, k):
    """gnc_xty_f32 with more row tiles than workers: against float64 with the relative bar of test_xty_matches_matmul (the
    column sums, formed over the same rows by the same workers, with the same bar), and bit for bit from run to run."""
    rows = _rows()["loop"]
    g = torch.Generator().manual_seed(m * 7 + k)
    a, b = torch.randn(rows, m, generator=g), torch.randn(rows, k, generator=g)
    c, cs = native.xty(a.to(DEV), b.to(DEV))
    ref, ref_s = a.double().t() @ b.double(), a.double().sum(0)
    assert _err(c, ref) / float(ref.abs().max()) < 2e-5
    assert _err(cs, ref_s) / float(ref_s.abs().max()) < 2e-5
    c2, cs2 = native.xty(a.to(DEV), b.to(DEV))
    assert torch.equal(c, c2) and torch.equal(cs, cs2)
