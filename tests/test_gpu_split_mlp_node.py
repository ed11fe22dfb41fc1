"""The node side of the weights-resident MLP kernel's split class (3-way bf16 split): the node processors
(class 2: the first Linear's two chunks stay fp32), the decoder and the single-Linear / dual projection (class 1), against
float64 on the host and against the exact fp32 path of the same launch (GNC_MLP_F32_EXACT=1, read once per process: each
arm runs every case once in one child process)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ROWS = 32 * 1024 * 2 + 4471  # tests/test_gpu_split_mlp.py's: every wave of a 256-CU grid owns tiles, the last tile is partial
FEW = 37                     # one partial tile, 2,047 idle waves
PARITY = 1e-5                # the project's parity bound

pytestmark = pytest.mark.gpu

# name -> (family, in width(s), out width)
CASES = {
    "node_res": ("node", 64, 64), "node": ("node", 64, 64),
    "dec1": ("dec", 64, 1), "dec3": ("dec", 64, 3),
    "proj64": ("proj", 64, 64), "proj48": ("proj", 48, 40),
}
KEYS = [(name, rows) for name in CASES for rows in (ROWS, FEW)]


def _case(name, rows):
    family, k, m = CASES[name]
    rng = np.random.default_rng(1000 * list(CASES).index(name) + rows % 997)
    u = lambda a, shape: rng.uniform(-1.0 / np.sqrt(a), 1.0 / np.sqrt(a), shape).astype(np.float32)  # noqa: E731
    c = dict(x=rng.standard_normal((rows, k)).astype(np.float32))
    if family == "node":
        c["agg"] = rng.standard_normal((rows, 64)).astype(np.float32)
        dims = [128, 64, 64, 64]
        c["ln"] = (rng.uniform(0.5, 1.5, (64,)).astype(np.float32), rng.uniform(-0.5, 0.5, (64,)).astype(np.float32))
    elif family == "dec":
        dims = [64, 64, 64, m]
    else:
        c["wa"], c["wb"] = u(k, (m, k)), u(k, (m, k))
        return c
    c["ws"] = [u(a, (b, a)) for a, b in zip(dims[:-1], dims[1:])]
    c["bs"] = [u(a, (b,)) for a, b in zip(dims[:-1], dims[1:])]
    return c


def _reference(name, c):
    """float64 on the host: the output (both outputs of a projection, side by side)."""
    family = CASES[name][0]
    f = lambda a: a.astype(np.float64)  # noqa: E731
    x = f(c["x"])
    if family == "proj":
        return np.concatenate([x @ f(c["wa"]).T, x @ f(c["wb"]).T], axis=1)
    ws, bs = [f(w) for w in c["ws"]], [f(b) for b in c["bs"]]
    a = np.concatenate([x, f(c["agg"])], axis=1) if family == "node" else x
    a = np.maximum(a @ ws[0].T + bs[0], 0.0)
    a = np.maximum(a @ ws[1].T + bs[1], 0.0)
    o = a @ ws[2].T + bs[2]
    if family == "dec":
        return o
    mu = o.mean(axis=1, keepdims=True)
    var = ((o - mu) ** 2).mean(axis=1, keepdims=True)
    y = (o - mu) / np.sqrt(var + 1e-5) * f(c["ln"][0]) + f(c["ln"][1])
    return y + x if name == "node_res" else y


def _forward(native, name, c, save=False):
    family = CASES[name][0]
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    x = t(c["x"])
    acts = [] if save else None
    if family == "proj":
        oa, ob = native.dual_projection(x, t(c["wa"]), t(c["wb"]))
        out = torch.cat([oa, ob], dim=1)
    elif family == "node":
        ws, bs = [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]
        out = native.mlp_forward([(x, None), (t(c["agg"]), None)], ws, bs, ln=(t(c["ln"][0]), t(c["ln"][1]), 1e-5),
                                 residual=x if name == "node_res" else None, save_act=acts)
    else:
        out = native.mlp_forward([(x, None)], [t(w) for w in c["ws"]], [t(b) for b in c["bs"]], save_act=acts)
    torch.cuda.synchronize()
    return out.cpu(), ([a.cpu() for a in acts] if save else None)


def _child(path):
    """Runs in a fresh process (the switch is read once).  Per case and row count: the output, a repeat, for the node
    processors the saving launch, for the projections the two single-Linear launches of the same products."""
    from graphnet_classifier_amd import native
    native.load_library()
    res = {}
    for name, rows in KEYS:
        c = _case(name, rows)
        out, _ = _forward(native, name, c)
        again, _ = _forward(native, name, c)
        r = {"out": out, "repeat_equal": torch.equal(out, again)}
        if CASES[name][0] == "node":
            out_s, acts = _forward(native, name, c, save=True)
            r["save_equal"], r["acts"] = torch.equal(out, out_s), acts
        if CASES[name][0] == "proj":
            x = torch.from_numpy(c["x"]).to(DEV)
            single = [native.mlp_forward([(x, None)], [torch.from_numpy(c[w]).to(DEV)], [None]) for w in ("wa", "wb")]
            r["single_equal"] = torch.equal(out, torch.cat(single, dim=1).cpu())
        res[f"{name}/{rows}"] = r
    torch.save(res, path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{exact: results of _child} - one child process per arm, shared by every test of the module."""
    tmp = tmp_path_factory.mktemp("split_node")
    got = {}
    for exact in (False, True):
        path = str(tmp / f"arm_{int(exact)}.pt")
        env = dict(os.environ)
        env.pop("GNC_MLP_F32_EXACT", None)
        if exact:
            env["GNC_MLP_F32_EXACT"] = "1"
        code = f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_gpu_split_mlp_node as m; m._child({path!r})"
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        got[exact] = torch.load(path)
    return got


@pytest.mark.parametrize("name,rows", KEYS)
def test_node_side_split_accuracy_and_bits(runs, name, rows):
    """Bars: the split arm's max-abs error against float64 is at most twice the exact arm's (the bar of
    tests/test_gpu_split_mlp.py) and at most the parity bound; both errors are printed."""
    ref = torch.from_numpy(_reference(name, _case(name, rows)))
    key = f"{name}/{rows}"
    err = {exact: float((r[key]["out"].double() - ref).abs().max()) for exact, r in runs.items()}
    print(f"{key}: max-abs error vs float64 split {err[False]:.3e}, fp32 exact {err[True]:.3e}")
    assert err[False] <= 2.0 * err[True]
    assert err[False] <= PARITY
    assert not torch.equal(runs[False][key]["out"], runs[True][key]["out"])  # the split instance did run
    for exact, r in runs.items():
        assert r[key]["repeat_equal"]                    # run-to-run determinism
        if CASES[name][0] == "node":
            assert r[key]["save_equal"]                  # saving changes no bit, in either class
        if CASES[name][0] == "proj" and not exact:
            assert r[key]["single_equal"]                # the dual launch and its two single-Linear twins: one class
    if CASES[name][0] == "node":
        if rows == ROWS:  # above the small-batch limit the node processors' backward reads what the forward saved
            assert len(runs[False][key]["acts"]) == 2 and len(runs[True][key]["acts"]) == 2
        for a, b in zip(runs[False][key]["acts"], runs[True][key]["acts"]):
            assert float((a - b).abs().max()) < PARITY
