"""Every launch shape of the weights-resident kernel's split class (3-way bf16 split), bit for bit against the
PARENT of the commit that software-pipelined the split between the MFMAs.

The fixtures (tests/golden/split_pipeline/) were recorded by tests/golden/make_split_pipeline_golden.py from the parent
commit's library, selected with GNC_LIB_PATH; split_pipeline.json names the commit.  tests/test_gpu_split_bits.py reaches most
of these launches only through the final [N, 1] output of the flagship forward; here every launch is compared directly:

* the cases of tests/test_gpu_split_mlp.py (W-split edge processor, encoder) and tests/test_gpu_split_mlp_node.py (node
  processors with and without the residual, decoder at out width 1 and 3, single and DUAL projection at 64 -> 64 and 48 -> 40);
* the W-split edge processor with the fused aggregation (the FULL instance at width 64), its aggregate-only twin, and the
  general-width instances (hidden 48, edge width 40: K-groups and fragments the look-ahead must not touch), with and
  without the fused aggregation;
* the training forward (SAVE instances): the saved post-activations of every hidden layer next to the output.

Each case runs at 37 rows (one partial tile) and at 70,007 rows (a wave walks several tiles).  Small outputs are stored
whole, the 70,007-row ones as SHA-256 of the bytes plus every 97th row (of a tensor that has to equal another one of its
case - the saving launch's output, the aggregate-only launch's aggregate, the single-Linear twins of DUAL - the digest only).  A row count is worth nothing if another kernel serves
it: every case first asks the library's own queries that the small-batch kernel does NOT take the launch and that the
weights-resident kernel does.  The class is decided by the shape alone, in the parent as in this build, so a case that fell
into the fp32 class would match its fixture without running any of the code under test: the whole case set therefore runs
once more in a child process with GNC_MLP_F32_EXACT=1 (read once per process), and every case asserts that its outputs
differ from that run's - the split class did serve it.

Further cases: the encoders that compute or read their rows in the kernel (`enc_ef`: the K6 prologue through
native.mlp_forward_edge_features, served only above the small-batch limit, so 70,007 rows only; `enc_n3`: a contiguous
[rows, 3] table read where it lies) and the FULL edge instance with row-ordered ADD tables (`edge_agg_rows`: its first
Linear runs outside the gather loop)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_gpu_split_mlp_node as node_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_pipeline")
DEV = "cuda"
ROWS = (37, 70007)
ROW_STEP = 97
WHOLE_BELOW = 1024  # tensors with fewer rows are stored whole
# tensors that must equal another tensor of the same case bit for bit (checked below): the fixtures keep their digest only
TWINS = {"save_out": "out", "save_agg": "agg", "only_agg": "agg", "single_a": "out_a", "single_b": "out_b"}

pytestmark = pytest.mark.gpu

# name -> (hidden width, edge width, fused aggregation, aggregate-only twin as well)
EDGE = {"edge": (64, 64, False, False), "edge_agg": (64, 64, True, True),
        "edge_gen": (48, 40, False, False), "edge_gen_agg": (48, 40, True, False), "edge_agg_rows": (64, 64, True, False)}
ENC = ("enc", "enc_ef", "enc_n3")
NODE = ("node_res", "node", "dec1", "dec3", "proj64", "proj48")
CASES = tuple(EDGE) + ENC + NODE
KEYS = [(name, rows) for name in CASES for rows in ROWS if not (name == "enc_ef" and rows < 1000)]
PRIMARY = ("out", "agg", "out_a", "out_b")  # what a launch computes through its split Linears


def _u(rng, fan_in, shape):
    return rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), shape).astype(np.float32)


def _edge_case(name, rows):
    hid, width, _, _ = EDGE[name]
    rng = np.random.default_rng(100 * list(EDGE).index(name) + rows % 991)
    nodes = 11 if rows < 1000 else 20011
    c = dict(x=rng.standard_normal((rows, width)).astype(np.float32), ps=rng.standard_normal((nodes, hid)).astype(np.float32),
             pd=rng.standard_normal((nodes, hid)).astype(np.float32), src=rng.integers(0, nodes, rows).astype(np.int32),
             dst=np.sort(rng.integers(0, nodes, rows)).astype(np.int32), nodes=nodes)
    dims = [width, hid, hid, width]
    c["ws"] = [_u(rng, a, (b, a)) for a, b in zip(dims[:-1], dims[1:])]
    c["bs"] = [_u(rng, a, (b,)) for a, b in zip(dims[:-1], dims[1:])]
    c["ln"] = (rng.uniform(0.5, 1.5, (width,)).astype(np.float32), rng.uniform(-0.5, 0.5, (width,)).astype(np.float32))
    return c


def _enc_case(name, rows):
    rng = np.random.default_rng(7000 + 10 * ENC.index(name) + rows % 991)
    k = 4 if name == "enc" else 3
    dims = [k, 64, 64, 64]
    nodes = 20011
    c = dict(x=rng.standard_normal((rows, k)).astype(np.float32))
    if name != "enc":  # (drawn here: the order the fixtures were recorded with)
        c.update(pos=rng.standard_normal((nodes, 2)).astype(np.float32), src=rng.integers(0, nodes, rows).astype(np.int32),
                 dst=np.sort(rng.integers(0, nodes, rows)).astype(np.int32))
    c["ws"] = [_u(rng, a, (b, a)) for a, b in zip(dims[:-1], dims[1:])]
    c["bs"] = [_u(rng, a, (b,)) for a, b in zip(dims[:-1], dims[1:])]
    c["ln"] = (rng.uniform(0.5, 1.5, (64,)).astype(np.float32), rng.uniform(-0.5, 0.5, (64,)).astype(np.float32))
    return c


def _t(a):
    return torch.from_numpy(a).to(DEV)


def _resident_serves(native, segs, ws, bs, ln, residual, rows, modes=None, vector_rows=True):
    """The library's own answers for this launch: the small-batch kernel does not take it, the weights-resident kernel does
    (gnc_mlp_operands_in_place_supported is 0 for exactly those two kernels)."""
    lib = native.load_library()
    s, w, b, res, rows, _ = native._prepare_mlp(segs, ws, bs, residual, rows, modes, vector_rows=vector_rows)
    dummy = torch.empty(max(rows, 1), w[-1].size(0), device=DEV)
    desc = native.make_mlp_desc(s, w, b, ln, "ReLU", 0.0, res, dummy, rows)
    small = lib.gnc_mlp_small_batch_supported(ctypes.byref(desc)) == 0
    return (not small) and lib.gnc_mlp_operands_in_place_supported(ctypes.byref(desc)) == 0


def run_case(native, name, rows, exact=False):
    """{tensor name: CPU tensor} of one case, and whether the weights-resident kernel serves every launch of it.  Shared with
    tests/golden/make_split_pipeline_golden.py.  ``exact``: the process runs the fp32 class (GNC_MLP_F32_EXACT=1)."""
    assert ("GNC_MLP_F32_EXACT" in os.environ) == exact
    got, routed = {}, True
    if name in EDGE:
        c = _edge_case(name, rows)
        _, _, agg, agg_only = EDGE[name]
        x, ws, bs = _t(c["x"]), [_t(w) for w in c["ws"]], [_t(b) for b in c["bs"]]
        ln = (_t(c["ln"][0]), _t(c["ln"][1]), 1e-5)
        dst = _t(c["dst"])
        segs = [(_t(c["ps"]), _t(c["src"])), (_t(c["pd"]), dst), (x, None)]
        if name == "edge_agg_rows":  # the ADD rows as row-ordered tables: no gather, the first Linear outside the gather loop
            segs = [(_t(c["ps"][c["src"]]), None), (_t(c["pd"][c["dst"]]), None), (x, None)]
        modes = [native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL]
        routed = _resident_serves(native, segs, ws, bs, ln, x, rows, modes)
        kw = dict(ln=ln, residual=x, rows=rows, modes=modes)
        if agg:
            rowptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV),
                                torch.cumsum(torch.bincount(dst.long(), minlength=c["nodes"]), 0)]).int()
            kw["aggregate"] = (dst, rowptr, c["nodes"])
        acts = []
        for tag, extra in (("", {}), ("save_", {"save_act": acts})) + ((("only_", {"agg_only": True}),) if agg_only else ()):
            r = native.mlp_forward(segs, ws, bs, **kw, **extra)
            out, a = r if agg else (r, None)
            if out is not None:  # (an aggregate-only launch returns no rows)
                got[tag + "out"] = out
            if agg:
                assert a is not None, "the fused aggregation did not serve this shape"
                got[tag + "agg"] = a
        if agg_only:
            assert "only_out" not in got, "the aggregate-only instance did not serve this shape"
        for l, a in enumerate(acts):
            got[f"save_act{l}"] = a
    elif name == "enc_ef":
        c = _enc_case(name, rows)
        ws, bs = [_t(w) for w in c["ws"]], [_t(b) for b in c["bs"]]
        ln = (_t(c["ln"][0]), _t(c["ln"][1]), 1e-5)
        out = native.mlp_forward_edge_features(_t(c["pos"]), _t(c["src"]), _t(c["dst"]), ws, bs, ln=ln)
        routed = out is not None  # None: gnc_mlp_edge_features_supported said no (only the weights-resident kernel serves this form)
        if routed:
            got["out"] = out
    elif name in ENC:
        c = _enc_case(name, rows)
        x, ws, bs = _t(c["x"]), [_t(w) for w in c["ws"]], [_t(b) for b in c["bs"]]
        ln = (_t(c["ln"][0]), _t(c["ln"][1]), 1e-5)
        routed = _resident_serves(native, [(x, None)], ws, bs, ln, None, rows, vector_rows=name != "enc_n3")
        acts = []
        got["out"] = native.mlp_forward([(x, None)], ws, bs, ln=ln, rows=rows)
        if name == "enc":  # (a saving launch of the [rows, 3] table goes through a zero-padded copy: not the EF = 2 instance)
            got["save_out"] = native.mlp_forward([(x, None)], ws, bs, ln=ln, rows=rows, save_act=acts)
        for l, a in enumerate(acts):
            got[f"save_act{l}"] = a
    else:
        family = node_cases.CASES[name][0]
        c = node_cases._case(name, rows)
        x = _t(c["x"])
        if family == "proj":
            wa, wb = _t(c["wa"]), _t(c["wb"])
            routed = _resident_serves(native, [(x, None)], [wa], [None], None, None, rows)
            got["out_a"], got["out_b"] = native.dual_projection(x, wa, wb)
            got["single_a"] = native.mlp_forward([(x, None)], [wa], [None])
            got["single_b"] = native.mlp_forward([(x, None)], [wb], [None])
        else:
            ws, bs = [_t(w) for w in c["ws"]], [_t(b) for b in c["bs"]]
            segs = [(x, None), (_t(c["agg"]), None)] if family == "node" else [(x, None)]
            ln = (_t(c["ln"][0]), _t(c["ln"][1]), 1e-5) if family == "node" else None
            res = x if name == "node_res" else None
            routed = _resident_serves(native, segs, ws, bs, ln, res, rows)
            got["out"] = native.mlp_forward(segs, ws, bs, ln=ln, residual=res)
            if family == "node":
                acts = []
                got["save_out"] = native.mlp_forward(segs, ws, bs, ln=ln, residual=res, save_act=acts)
                for l, a in enumerate(acts):
                    got[f"save_act{l}"] = a
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}, routed


def sha256(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def stored_rows(t):
    """What the fixture keeps of a tensor: all of it when small, every ROW_STEP-th row otherwise."""
    return t if t.shape[0] < WHOLE_BELOW else t[::ROW_STEP]


def fixture_path(name, rows):
    return os.path.join(GOLDEN, f"{name}_{rows}.npz")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(GOLDEN, "split_pipeline.json")) as f:
        return json.load(f)


def _exact_child(path):
    """Runs in a fresh process with GNC_MLP_F32_EXACT=1: the digests of every case's primary outputs on the fp32 class."""
    from graphnet_classifier_amd import native
    native.load_library()
    res = {}
    for name, rows in KEYS:
        got, _ = run_case(native, name, rows, exact=True)
        res[f"{name}/{rows}"] = {k: sha256(v) for k, v in got.items() if k in PRIMARY}
    with open(path, "w") as f:
        json.dump(res, f)


@pytest.fixture(scope="module")
def exact_digests(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("split_pipeline") / "exact.json")
    env = dict(os.environ, GNC_MLP_F32_EXACT="1")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_gpu_split_pipeline_bits as m; m._exact_child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("name,rows", KEYS)
def test_launch_bits_match_parent(meta, exact_digests, name, rows):
    from graphnet_classifier_amd import native
    native.load_library()
    got, routed = run_case(native, name, rows)
    assert routed, "not served by the weights-resident kernel: the case says nothing about it"
    # ... on the split class: every primary output differs from the fp32 class's of the same launch
    primary = [k for k in got if k in PRIMARY]
    assert primary and sorted(primary) == sorted(exact_digests[f"{name}/{rows}"])
    for k in primary:
        assert sha256(got[k]) != exact_digests[f"{name}/{rows}"][k], f"{k}: the fp32 class's bits - the split class did not serve this case"
    want_meta = meta["cases"][f"{name}/{rows}"]
    assert sorted(got) == sorted(want_meta), (sorted(got), sorted(want_meta))
    with np.load(fixture_path(name, rows)) as z:
        want = {k: torch.from_numpy(z[k]) for k in z.files}
    assert sorted(want) == sorted(k for k in got if k not in TWINS)
    for k in sorted(got):
        g, w = stored_rows(got[k]), want[TWINS.get(k, k)]
        assert list(got[k].shape) == want_meta[k]["shape"] and g.shape == w.shape and g.dtype == w.dtype == torch.float32
        differ = int((g.view(torch.int32) != w.view(torch.int32)).sum())
        digest = sha256(got[k])
        print(f"{name}/{rows} {k}: {differ} of {g.numel()} stored values differ from the parent's; sha256 "
              f"{'equal' if digest == want_meta[k]['sha256'] else 'DIFFERS'}")
        assert differ == 0, k
        assert digest == want_meta[k]["sha256"], k
    # twins inside the launch set (no fixture needed): saving changes no bit, the aggregate-only launch forms the storing
    # launch's aggregate, the DUAL launch computes what two single-Linear launches compute
    for b, a in TWINS.items():
        if b in got:
            assert torch.equal(got[a], got[b]), (a, b)
