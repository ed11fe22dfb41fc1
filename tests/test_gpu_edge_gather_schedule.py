"""The W-split edge processor with the fused aggregation (all widths 64, three Linears, LayerNorm, inference: the FULL
instances of the weights-resident kernel) after its gather requests were moved to the front of the first Linear.
Only the place of loads and waits in the instruction stream changed, so every result is held bit for bit:

(a) e' and the aggregate of the storing launch, and the aggregate of the aggregate-only launch, equal those of the same launch
    run with GNC_MLP_NO_FULL64=1 in a fresh child process (the switch is read once): the general-width instance, whose
    request schedule is the even one;
(b) the aggregate equals K1 (scatter_sum_csr) over the stored e';
(c) the aggregate-only launch forms the storing launch's aggregate;
(d) e' is within the tolerance of tests/test_gpu_split_mlp.py (4e-6, same weight and input distributions) of a float64
    evaluation of the same formula.

Row counts: 37 (one full and one partial tile), 4,099, and 70,007 (2,188 tiles on 2,048 waves: some waves walk two tiles,
others one).  Node tables of 5 rows (every gather id repeated many times) and of 1,000 rows; the ids hit the first and the
last row of the table on both sides.  Edges are destination-sorted, with destinations of 0, 1, 33 and 70 edges (70 edges span
more than two tiles and cross wave ranges; the 37-row cases have room for 0, 1 and 33 only)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_gpu_split_mlp as split_mlp
from tests.test_gpu_split_pipeline_bits import _resident_serves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ROWS = (37, 4099, 70007)
NODES = (5, 1000)
KEYS = [(rows, nodes) for rows in ROWS for nodes in NODES]
TOL = 4e-6  # tests/test_gpu_split_mlp.py, the 'edge' shape

pytestmark = pytest.mark.gpu


def _degrees(rng, rows, nodes):
    """Edges per destination: 70 (where they fit), 0, 1, 33 in front, the last node at least one, the rest at random."""
    deg = np.zeros(nodes, dtype=np.int64)
    deg[:4] = (70 if rows >= 70 + 35 else 1), 0, 1, 33
    deg[-1] = 1
    left = rows - int(deg.sum())
    assert left >= 0
    if nodes == 5:
        deg[-1] += left
    else:
        deg[4:] += rng.multinomial(left, np.full(nodes - 4, 1.0 / (nodes - 4)))
    assert deg.sum() == rows and deg[0] >= 1 and deg[-1] >= 1
    return deg


def _case(rows, nodes):
    rng = np.random.default_rng(1000 * nodes + rows)
    deg = _degrees(rng, rows, nodes)
    src = rng.integers(0, nodes, rows).astype(np.int32)
    src[0], src[1], src[-1] = 0, nodes - 1, nodes - 1
    c = dict(x=rng.standard_normal((rows, 64)).astype(np.float32), ps=rng.standard_normal((nodes, 64)).astype(np.float32),
             pd=rng.standard_normal((nodes, 64)).astype(np.float32), src=src,
             dst=np.repeat(np.arange(nodes), deg).astype(np.int32), deg=deg)
    c["ws"], c["bs"], c["ln"] = split_mlp._weights(rng, 64)
    return c


def _run(native, c):
    """{e, agg, only_agg, k1} of one case on the CPU, and whether the weights-resident kernel serves the launch."""
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    rows, nodes = c["x"].shape[0], c["ps"].shape[0]
    x, ws, bs = t(c["x"]), [t(w) for w in c["ws"]], [t(b) for b in c["bs"]]
    ln = (t(c["ln"][0]), t(c["ln"][1]), 1e-5)
    dst = t(c["dst"])
    segs = [(t(c["ps"]), t(c["src"])), (t(c["pd"]), dst), (x, None)]
    modes = [native.SEG_ADD, native.SEG_ADD, native.SEG_MATMUL]
    routed = _resident_serves(native, segs, ws, bs, ln, x, rows, modes)
    rowptr = t(np.concatenate([[0], np.cumsum(c["deg"])]).astype(np.int32))
    kw = dict(ln=ln, residual=x, rows=rows, modes=modes, aggregate=(dst, rowptr, nodes))
    e, agg = native.mlp_forward(segs, ws, bs, **kw)
    only_e, only_agg = native.mlp_forward(segs, ws, bs, **kw, agg_only=True)
    assert agg is not None and only_agg is not None, "the fused aggregation did not serve this shape"
    k1 = native.scatter_sum_csr(e, rowptr, None, nodes)
    torch.cuda.synchronize()
    return dict(e=e.cpu(), agg=agg.cpu(), only_agg=only_agg.cpu(), k1=k1.cpu()), routed, only_e is None


def _general_child(path):
    """Runs in a fresh process with GNC_MLP_NO_FULL64=1: every case on the general-width instance."""
    from graphnet_classifier_amd import native
    native.load_library()
    assert "GNC_MLP_NO_FULL64" in os.environ
    res = {}
    for rows, nodes in KEYS:
        got, routed, _ = _run(native, _case(rows, nodes))
        assert routed
        res[(rows, nodes)] = got
    torch.save(res, path)


@pytest.fixture(scope="module")
def general(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("edge_gather") / "general.pt")
    env = dict(os.environ, GNC_MLP_NO_FULL64="1")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); import tests.test_gpu_edge_gather_schedule as m; m._general_child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return torch.load(path)


def _differ(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    return int((a.view(torch.int32) != b.view(torch.int32)).sum())


@pytest.mark.parametrize("rows,nodes", KEYS)
def test_front_loaded_gathers_change_no_bit(general, rows, nodes):
    from graphnet_classifier_amd import native
    native.load_library()
    assert "GNC_MLP_NO_FULL64" not in os.environ and "GNC_MLP_F32_EXACT" not in os.environ
    c = _case(rows, nodes)
    got, routed, only_dropped_rows = _run(native, c)
    assert routed, "not served by the weights-resident kernel: the case says nothing about it"
    assert only_dropped_rows, "the aggregate-only instance did not serve this shape"
    want = general[(rows, nodes)]
    err = float((got["e"].double() - torch.from_numpy(split_mlp._reference("edge", c))).abs().max())
    figures = {"a: e' vs general": _differ(got["e"], want["e"]), "a: agg vs general": _differ(got["agg"], want["agg"]),
               "a: aggregate-only agg vs general": _differ(got["only_agg"], want["agg"]),
               "b: agg vs K1": _differ(got["agg"], got["k1"]), "c: aggregate-only agg vs storing": _differ(got["only_agg"], got["agg"])}
    print(f"{rows} rows, {nodes} nodes: values that differ {figures}; max-abs error of e' vs float64 {err:.3e}")
    for what, n in figures.items():
        assert n == 0, what
    assert err <= TOL
