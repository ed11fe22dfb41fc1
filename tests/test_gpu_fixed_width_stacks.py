"""The fixed-width instances of the weights-resident MLP kernel for c3's plain stacks (FULL with one MATMUL step
and no ADD segments - the edge encoder with the edge-feature prologue, the node encoder on the [rows, 3] table, the same
stack on a 64-wide segment) against the general-width instances of the same launches (GNC_MLP_NO_FULL64=1), against the
exact fp32 class (GNC_MLP_F32_EXACT=1) and against float64 on the host.  The decoder has NO fixed-width instance (DESIGN.md
K4 says why): its case runs the general instance in both arms and only pins the present path.  The switches are read once per process:
each arm runs every case once (and a repeat) in one child process, in the pattern of tests/test_gpu_split_mlp_node.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ROWS = 70007   # the neighbours' row count: on a 256-CU grid some waves walk two tiles, the last tile is partial
FEW = 37       # one partial tile, every other wave idle
PARITY = 1e-5  # the project's parity bound
NODES = 20011

pytestmark = pytest.mark.gpu

# name -> (widths of the stack, LayerNorm, served by the split class when the weights-resident kernel takes the launch)
CASES = {
    "enc_ef": ([3, 64, 64, 64], True, True),    # MLP.forward_edge_features: EF = 1
    "enc_n3": ([3, 64, 64, 64], True, True),    # a contiguous [rows, 3] table: EF = 2
    "enc_64": ([64, 64, 64, 64], True, False),  # the same stack on a 64-wide segment: fp32 MFMA in either class
    "dec_1": ([64, 64, 64, 1], False, True),    # the decoder: the general instance in either arm (no fixed-width one)
}
KEYS = [(name, rows) for name in CASES for rows in (FEW, ROWS)]
ARMS = {"default": None, "general": "GNC_MLP_NO_FULL64", "exact": "GNC_MLP_F32_EXACT"}


def _case(name, rows):
    dims, has_ln, _ = CASES[name]
    rng = np.random.default_rng(31000 + 100 * list(CASES).index(name) + rows % 991)
    u = lambda a, shape: rng.uniform(-1.0 / np.sqrt(a), 1.0 / np.sqrt(a), shape).astype(np.float32)  # noqa: E731
    c = {}
    if name == "enc_ef":
        c["pos"] = rng.standard_normal((NODES, 2)).astype(np.float32)
        src = rng.integers(0, NODES, rows)
        dst = np.sort(rng.integers(0, NODES, rows))
        dst[-1] = NODES  # one id outside the table, clamped by the caller as the model's topology does
        c["src"], c["dst"] = src.astype(np.int32), np.minimum(dst, NODES - 1).astype(np.int32)
    else:
        c["x"] = rng.standard_normal((rows, dims[0])).astype(np.float32)
    c["ws"] = [u(a, (b, a)) for a, b in zip(dims[:-1], dims[1:])]
    c["bs"] = [u(a, (b,)) for a, b in zip(dims[:-1], dims[1:])]
    if has_ln:
        c["ln"] = (rng.uniform(0.5, 1.5, (dims[-1],)).astype(np.float32), rng.uniform(-0.5, 0.5, (dims[-1],)).astype(np.float32))
    return c


def _reference(name, c):
    """float64 on the host."""
    f = lambda a: a.astype(np.float64)  # noqa: E731
    if name == "enc_ef":
        d = f(c["pos"])[c["dst"]] - f(c["pos"])[c["src"]]
        a = np.concatenate([d, np.abs(d).sum(axis=1, keepdims=True)], axis=1)
    else:
        a = f(c["x"])
    ws, bs = [f(w) for w in c["ws"]], [f(b) for b in c["bs"]]
    a = np.maximum(a @ ws[0].T + bs[0], 0.0)
    a = np.maximum(a @ ws[1].T + bs[1], 0.0)
    o = a @ ws[2].T + bs[2]
    if "ln" not in c:
        return o
    mu = o.mean(axis=1, keepdims=True)
    var = ((o - mu) ** 2).mean(axis=1, keepdims=True)
    return (o - mu) / np.sqrt(var + 1e-5) * f(c["ln"][0]) + f(c["ln"][1])


def _t(a):
    return torch.from_numpy(a).to(DEV)


def _encoder_module(c):
    """The edge encoder as the model holds it, with the case's parameters."""
    from graphnet_classifier_amd.MLP import MLP
    enc = MLP(3, 64, hidden_dim=64, hidden_layers=2).eval()
    with torch.no_grad():
        for m, w, b in zip(enc._linears(), c["ws"], c["bs"]):
            m.weight.copy_(_t(w))
            m.bias.copy_(_t(b))
        enc.model[-1].weight.copy_(_t(c["ln"][0]))
        enc.model[-1].bias.copy_(_t(c["ln"][1]))
    return enc


def _forward(native, name, c):
    """(output on the host, does the weights-resident kernel serve the launch - the library's own answer)."""
    from graphnet_classifier_amd import functional as Fn
    if name == "enc_ef":
        enc, pos, src, dst = _encoder_module(c), _t(c["pos"]), _t(c["src"]), _t(c["dst"])
        with torch.no_grad():
            out = enc.forward_edge_features(pos, src, dst)
            routed = out is not None  # None below the small-batch limit: the model's own fall-back then
            if out is None:
                out = enc.forward_segments([(Fn.edge_features(pos, src, dst), None)])
    else:
        x, ws, bs = _t(c["x"]), [_t(w) for w in c["ws"]], [_t(b) for b in c["bs"]]
        ln = (_t(c["ln"][0]), _t(c["ln"][1]), 1e-5) if "ln" in c else None
        lib = native.load_library()
        s, w, b, res, rows, _ = native._prepare_mlp([(x, None)], ws, bs, None, None, None, vector_rows=name != "enc_n3")
        desc = native.make_mlp_desc(s, w, b, ln, "ReLU", 0.0, res, torch.empty(rows, w[-1].size(0), device=DEV), rows)
        # (gnc_mlp_operands_in_place_supported is 0 for the small-batch kernel and the weights-resident kernel alone)
        routed = lib.gnc_mlp_small_batch_supported(ctypes.byref(desc)) != 0 and \
            lib.gnc_mlp_operands_in_place_supported(ctypes.byref(desc)) == 0
        out = native.mlp_forward([(x, None)], ws, bs, ln=ln)
    torch.cuda.synchronize()
    return out.cpu(), routed


def _child(path):
    """Runs in a fresh process (the switches are read once): per case and row count the output, a repeat, the routing."""
    from graphnet_classifier_amd import native
    native.load_library()
    res = {}
    for name, rows in KEYS:
        c = _case(name, rows)
        out, routed = _forward(native, name, c)
        again, _ = _forward(native, name, c)
        res[f"{name}/{rows}"] = {"out": out, "repeat_equal": torch.equal(out, again), "routed": routed}
    torch.save(res, path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{arm: results of _child} - one child process per arm, shared by every test of the module."""
    tmp = tmp_path_factory.mktemp("fixed_width")
    got = {}
    for arm, switch in ARMS.items():
        path = str(tmp / f"arm_{arm}.pt")
        env = dict(os.environ)
        for s in ARMS.values():
            if s:
                env.pop(s, None)
        if switch:
            env[switch] = "1"
        code = f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_gpu_fixed_width_stacks as m; m._child({path!r})"
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
        got[arm] = torch.load(path)
    return got


@pytest.fixture(scope="module")
def references():
    return {f"{name}/{rows}": torch.from_numpy(_reference(name, _case(name, rows))) for name, rows in KEYS}


@pytest.mark.parametrize("name,rows", KEYS)
def test_fixed_width_stack_bits_and_accuracy(runs, references, name, rows):
    """The fixed-width and the general-width instance agree bit for bit; every arm repeats itself; where the weights-resident
    kernel serves a launch of the split class, the default arm is not the exact fp32 arm (the 64-wide stack is fp32 MFMA in
    either class by the launcher's rule, and equals it); the error against float64 is within the parity bound."""
    key = f"{name}/{rows}"
    got = {arm: r[key] for arm, r in runs.items()}
    err = {arm: float((g["out"].double() - references[key]).abs().max()) for arm, g in got.items()}
    print(f"{key}: routed {got['default']['routed']}, max-abs error vs float64 " + ", ".join(f"{a} {e:.3e}" for a, e in err.items()))
    assert got["default"]["out"].shape == references[key].shape
    assert torch.equal(got["default"]["out"], got["general"]["out"])
    for g in got.values():
        assert g["repeat_equal"]
    if rows == ROWS:
        assert got["default"]["routed"]  # above the small-batch limit the weights-resident kernel takes every case
    if got["default"]["routed"]:
        assert torch.equal(got["default"]["out"], got["exact"]["out"]) == (not CASES[name][2])
    assert err["default"] <= PARITY
